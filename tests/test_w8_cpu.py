"""FP8 (E4M3) decoder weights on the host side: the quantiser (indextts/utils/quant.py), the FP8 GEMM entry points of the C ABI
(symbols, sizes, planner, refusals -- no GPU needed: validation comes first) and the precision resolution of the public surface.

Quantiser bounds.  scale[n] is fp32(max_k |W[k, n]| / 448); the codes are the round-to-nearest-even E4M3 encoding of W / scale,
rounded once from float64, so |W / scale - decode(code)| is at most half the E4M3 grid spacing at that value (2^-9 below 2^-6, else
2^(e - 3) with e the value's binade) -- except where the clamp to +-448 acted: the fp32 rounding of the scale can put the column
maximum at 448 (1 +- 2^-24), which is clamped, an excess of at most 448 * 2^-24 in units of the scale.  The column maximum
therefore maps to code 0x7e / 0xfe (+-448) -- the exact part of its round trip, asserted for every column -- and dequantises to
448 * scale: that is the maximum itself, bit for bit, wherever amax / 448 is an fp32 value (asserted on such columns), and within
the scale's fp32 rounding, 2^-24 relative, otherwise (a scale stored in fp32 cannot do better)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_F8 = hasattr(torch, "float8_e4m3fn")


def columns():
    """float64 [K, N]: seeded random columns of many magnitudes and the adversarial ones."""
    g = torch.Generator().manual_seed(11)
    K = 257
    w = torch.randn(K, 24, generator=g, dtype=torch.float64) * torch.logspace(-6, 3, 24, dtype=torch.float64)
    zero = torch.zeros(K, 1, dtype=torch.float64)
    outlier = torch.randn(K, 1, generator=g, dtype=torch.float64) * 1e-2
    outlier[17] = 300.0                                              # one huge outlier: everything else lands in the subnormals / zero
    edge = torch.randn(K, 1, generator=g, dtype=torch.float64)
    edge[3], edge[4] = 7.25, -7.25                                   # +-448 . scale: the column's maximum, both signs
    tiny = torch.randn(K, 1, generator=g, dtype=torch.float64)
    tiny[5:40] = torch.linspace(-1, 1, 35, dtype=torch.float64)[:, None] * tiny.abs().max() / 448 * 2.0 ** -10   # below half the smallest subnormal
    grid = torch.zeros(K, 1, dtype=torch.float64)                    # exact grid values and exact midpoints (ties) at scale 1
    from indextts.utils import quant
    vals = quant.decode_e4m3(torch.arange(127, dtype=torch.uint8))
    mids = (vals[:-1] + vals[1:]) / 2
    grid[:127, 0], grid[127:253, 0] = vals, -mids
    return torch.cat([w, zero, outlier, edge, tiny, grid], 1)


def test_quantiser_properties():
    from indextts.utils import quant
    w = columns()
    codes, scale = quant.quantize_e4m3_cols(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[1],)
    assert not ((codes & 0x7f) == 0x7f).any(), "a NaN code was produced"
    amax = w.abs().amax(0)
    assert torch.equal(scale, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float())
    assert scale[24].item() == 1.0 and (codes[:, 24] == 0).all()     # the all-zero column
    deq = quant.dequantize(codes, scale)
    assert deq.dtype == torch.float64
    x = w / scale.double()
    _, ex = torch.frexp(x.abs())
    half_step = torch.ldexp(torch.ones_like(x), torch.clamp(ex - 1, min=-6) - 3) / 2
    clamp_excess = torch.clamp(x.abs() - 448.0, min=0.0)
    assert (clamp_excess <= 448.0 * 2.0 ** -24).all()
    err = (x - quant.decode_e4m3(codes)).abs()
    assert (err <= half_step + clamp_excess).all(), (err - half_step).max()
    assert ((w - deq).abs() <= (half_step + clamp_excess) * scale.double()).all()
    # the column maximum maps to +-448 and comes back within the scale's fp32 rounding
    top = w.abs().argmax(0)
    cols = torch.arange(w.shape[1])
    nz = amax > 0
    assert ((codes[top, cols] & 0x7f)[nz] == 0x7e).all()
    assert ((deq[top, cols] - w[top, cols]).abs()[nz] <= 2.0 ** -24 * amax[nz]).all()
    # ... and EXACTLY wherever an exact round trip exists: 448 . fp32(amax / 448) is amax itself only if amax / 448 is an fp32
    # value (the grid column, amax = 448; the column appended here, amax = 448 . 2^-5); there the value comes back bit for bit
    extra = w[:, :1] * (13.0 / amax[0])
    extra[top[0], 0] = -14.0
    wx = torch.cat([w, extra], 1)
    cx, sx = quant.quantize_e4m3_cols(wx)
    ax = wx.abs().amax(0)
    exact = (sx.double() * 448.0 == ax) & (ax > 0)
    assert exact[28] and exact[-1] and sx[-1].item() == 2.0 ** -5
    tx = wx.abs().argmax(0)
    cx_cols = torch.arange(wx.shape[1])
    assert torch.equal(quant.dequantize(cx, sx)[tx, cx_cols][exact], wx[tx, cx_cols][exact])
    assert torch.equal(codes[3, 26], torch.tensor(0x7e, dtype=torch.uint8)) and codes[4, 26].item() == 0xfe
    # values below half the smallest subnormal vanish (a signed zero), the outlier column keeps its outlier
    assert ((codes[5:40, 27] & 0x7f) == 0).all() and (codes[17, 25] & 0x7f) == 0x7e
    # ties go to the even code
    g = codes[127:253, 28].long() & 0x7f
    assert (g % 2 == 0).all() and (codes[127:253, 28] >= 128).all()
    # deterministic, and independent of the input's float width where fp32 holds the values
    c2, s2 = quant.quantize_e4m3_cols(w.clone())
    assert torch.equal(c2, codes) and torch.equal(s2, scale)
    w32 = w.float()
    c3, s3 = quant.quantize_e4m3_cols(w32)
    c4, s4 = quant.quantize_e4m3_cols(w32.double())
    assert torch.equal(c3, c4) and torch.equal(s3, s4)


@pytest.mark.skipif(not HAS_F8, reason="this torch has no float8_e4m3fn")
def test_rounding_is_torchs_e4m3fn_cast():
    from indextts.utils import quant
    w = columns()
    codes, scale = quant.quantize_e4m3_cols(w)
    x = (w / scale.double()).clamp(-448.0, 448.0)
    assert torch.equal(codes, x.to(torch.float8_e4m3fn).view(torch.uint8))
    # and the decode table is the format's: all 254 non-NaN codes
    allc = torch.arange(256, dtype=torch.uint8)
    f8 = allc.view(torch.float8_e4m3fn).double()
    ok = ~torch.isnan(f8)
    assert int(ok.sum()) == 254 and torch.equal(quant.decode_e4m3(allc)[ok], f8[ok])


def test_abi_symbols_sizes_plan_and_refusals():
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_abi_version() == 10
    main = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert re.search(r"#define ITTS_ABI_VERSION (\d+)", main).group(1) == "10"
    txt = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    syms = ["itts_gemm_skinny_w8", "itts_pack_weight_w8", "itts_packed_bytes_w8", "itts_skinny_plan_w8"]
    declared = set(re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", txt))
    plain = ctypes.CDLL(nat.LIB_PATH)
    assert all(s_ in declared and hasattr(plain, s_) and s_ in nat.EXPORTED_SYMBOLS for s_ in syms)
    # the struct both GEMM entry points take: its fields, in the header's order
    decl = txt[txt.index("typedef struct itts_skinny_args {"):txt.index("} itts_skinny_args;")]
    order = [n for line in decl.split("{", 1)[1].split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert order == [f[0] for f in nat.SkinnyArgs._fields_] and order[-1] == "w_scale"
    assert "const itts_skinny_args* a" in txt[txt.index("int itts_gemm_skinny_w8("):]
    # packed bytes: ceil(N / 16) * ceil(K / 64) KiB
    for K in (64, 96, 1280):
        for N in (16, 20, 8194):
            assert L.itts_packed_bytes_w8(K, N) == -(-N // 16) * -(-K // 64) * 1024
    assert L.itts_packed_bytes_w8(1280, 3840) * 2 == L.itts_packed_bytes(1, 1280, 3840, nat.BF16)
    # the planner on the decode step's own shapes (D = 1280: QKV', out-projection, FC', FC2, head), at the row counts the engine
    # launches them with: one round of the 256 CUs
    D, V = 1280, 8194
    for dtype in (torch.bfloat16, torch.float16):
        for B in (1, 3, 16, 32, 33, 64, 96):
            rc, ro = (32, 32) if B > 32 else (0, 16)
            for N, K, rpw, fold in ((3 * D, D, rc, True), (D, D, ro, False), (4 * D, D, rc, True), (D, 4 * D, ro, False), (V, D, 0, False)):
                p = nat.skinny_plan_w8(dtype, B, N, K, rpw, fold)
                gx, gy, gz = p["grid"]
                assert gy == 1 and gx * gz <= 256, (B, N, K, p)
                assert gx * p["tiles_per_wg"] >= -(-N // 16) and p["waves"] * p["ksteps_per_wave"] >= -(-K // 64)
                assert p["lds"] <= 160 * 1024
    # refusals name the entry point and launch nothing
    a = nat.SkinnyArgs()
    assert L.itts_gemm_skinny_w8(ctypes.byref(a), None) == 1 and b"itts_gemm_skinny_w8: null" in L.itts_last_error()
    a.wp = a.x = a.y = a.w_scale = 0x1000        # never dereferenced: every call below fails its checks
    a.dtype, a.M, a.N, a.K, a.epi = nat.BF16, 4, 64, 64, nat.EPI_STORE

    def refused(word, **kw):
        b = nat.SkinnyArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        assert L.itts_gemm_skinny_w8(ctypes.byref(b), None) == 1
        msg = L.itts_last_error()
        assert msg.startswith(b"itts_gemm_skinny_w8:") and word in msg, msg
    refused(b"ksplit", ksplit=2)
    refused(b"bf16 or f16", dtype=nat.F32)
    refused(b"w_scale", w_scale=None)
    refused(b"epilogue", epi=nat.EPI_RELU_AFFINE_STORE)
    refused(b"epilogue", epi=nat.EPI_RELU_AFFINE_TANH_STORE)
    refused(b"epilogue", epi=nat.EPI_SLAB_F32)
    refused(b"epilogue", epi=nat.EPI_SILU_STORE)
    refused(b"K % 32", K=48)
    # ... and the 16-bit entry point never reads an FP8 image as 16-bit weights
    assert L.itts_gemm_skinny(ctypes.byref(a), None) == 1 and L.itts_last_error().startswith(b"itts_gemm_skinny: w_scale")
    out = (ctypes.c_int * 8)()
    assert L.itts_skinny_plan_w8(nat.F32, 4, 64, 64, 0, 0, out) == 1 and b"itts_skinny_plan_w8" in L.itts_last_error()


def test_precision_resolution():
    from indextts import infer
    assert infer._resolve_gpt_precision("fp8") == (torch.bfloat16, "fp8", False)
    assert infer._resolve_dtype("fp8") == torch.bfloat16
    assert infer._resolve_gpt_precision("int8") == (torch.bfloat16, None, True)          # unchanged: bf16 weights and the warning
    assert infer._resolve_gpt_precision("int4") == (torch.bfloat16, None, True)
    assert infer._resolve_gpt_precision("fp8", {"enabled": True}) == (torch.bfloat16, None, True)
    assert infer._resolve_gpt_precision("bf16") == (torch.bfloat16, None, False)
    assert infer._resolve_gpt_precision("fp16") == (torch.float16, None, False)
    assert infer._resolve_gpt_precision("fp32") == (torch.float32, None, False)
    assert infer._resolve_gpt_precision("bf16", None) == (torch.bfloat16, None, False)
