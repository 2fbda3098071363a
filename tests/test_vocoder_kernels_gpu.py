"""fp64 parity of every 16-bit vocoder kernel form, element by element, with bounds derived from where each form rounds.

Every case runs one HIP kernel on operands already rounded to the storage type and compares it with a float64
evaluation of the same operation on those operands, on the GPU (explicit shifted sums; no MIOpen, no host BLAS).  Each
case also reads `itts_last_kernel()` and asserts the form it names, so that a change to the dispatch code cannot silently
move a case off the form it is meant to pin.

Bounds (per element, never one global max-abs figure):

  Convolutions (every form accumulates the exact 16-bit products in fp32 and rounds once to the storage type):
      |y - ref| <= ulp_T(ref) + 2^-21 * S,   S = |scale| * (sum_{j,c} |x w| + |bias| + |bias2| + |resid|) + |y_prev|
  ulp_T(ref) covers the final rounding (half an ulp) with half an ulp to spare; 2^-21 * S covers the fp32 sums (a k-ordered
  fp32 chain measures 0.75-3.5e-7 * sum|a b| at K = 1k-4k against an fp64 reference; 2^-21 = 4.8e-7) and the epilogue's
  fp32 roundings (bias, residual, the fused multiply-add with the running sum).

  Activation (see `act_bound` for the derivation): half an ulp of the storage type at the reference value (the single
  final rounding) plus twice the fp32-level error budget; the MFMA form's extra fp16 rounding of the snake output s is
  part of the REFERENCE (the reference rounds s to fp16 exactly where the kernel does), and an element only gets an
  allowance for it where its fp64 s lies so close to an fp16 rounding midpoint that the kernel's fp32 s may round the
  other way.

Negative controls: for each kernel family, the same assertion must FAIL against a reference that is wrong in one small
way (input shifted by one row at a tile boundary; zero instead of replicate padding at the sequence end; one filter or
weight tap off by 2^-9 relative; alpha and beta swapped or two channels exchanged).  The controls only re-evaluate the
reference on the host side of the test; the kernel runs once.

`test_production_*` record the signatures and forms of an eager fp16 BigVGAN.forward at production geometry (batch 32,
140 latent frames, synthetic full-size checkpoint), pin every signature to the fp64 reference, and check that every form
the forward used is one that the edge matrix below pins (run the whole file: the edge tests fill that set).
"""
import math

import numpy as np
import pytest
import torch

import weights
from fp64_check import check, excess, must_fail, ulp  # noqa: F401  (shared with test_decode_kernels_gpu.py)
from vocoder_refs import (EHW, EPI_MATRIX, EPIS, act_bound, act_ref, conv_bound, conv_ref, perturbed_filter, perturbed_tap,  # noqa: F401
                          shifted_rows, swapped_last, ups_slice)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
PINNED = set()                            # forms the edge matrix below has pinned to fp64 (read by the coverage test)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fir():
    from indextts.BigVGAN.models import kaiser_sinc_filter
    f = kaiser_sinc_filter()
    return f, f


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def form(nat, expect=None, pin=True):
    f = nat.last_kernel()
    if expect is not None:
        assert f == expect or (expect.endswith("*") and f.startswith(expect[:-1])), f"dispatched {f!r}, expected {expect!r}"
    if pin:
        PINNED.add(f)
    return f


# ------------------------------------------------------------------------------------------------- convolution
# conv_ref, conv_bound, EPIS / EPI_MATRIX and the control builders: tests/vocoder_refs.py


def run_conv(nat, dtype, B, T, C, N, k, d, epi, seed, vr=None, controls=False, expect=None, pin=True):
    """One 'same' convolution (off0 = -(k-1)d/2) with the epilogue `epi`; asserts fp64 parity, returns the form."""
    x = rnd(B, T, C, seed=seed).to(dtype)
    w = (rnd(k, C, N, seed=seed + 1) / math.sqrt(C * k)).to(dtype)
    bias = (rnd(N, seed=seed + 2) * 0.1).float()
    off0 = -((k - 1) * d // 2)
    has_r, acc, scale, has_b2 = EPIS[epi]
    kw, rk = {}, {}
    y = torch.full((B, T, N), 7.0, dtype=dtype, device=DEV)
    if has_r:
        kw["resid"] = rk["resid"] = rnd(B, T, N, seed=seed + 3).to(dtype)
    if acc:
        y = rnd(B, T, N, seed=seed + 4).to(dtype)
        rk["yprev"] = y.clone()
        kw["accumulate"] = True
    if scale != 1.0:
        kw["scale"] = rk["scale"] = scale
    if has_b2:
        kw["bias2"] = rk["bias2"] = (rnd(B, N, seed=seed + 5) * 0.1).float()
    wp = nat.pack_weight(w)
    nat.gemm_conv(dtype, B, T, T, C, N, wp, x, y, taps=k, off0=off0, dil=d, bias=bias, valid_rows=vr, **kw)
    f = form(nat, expect, pin)
    what = f"{f} B={B} T={T} C={C} N={N} k={k} d={d} {epi}" + ("" if vr is None else f" lens={vr.tolist()}")
    ref, mag = conv_ref(x, w, k, off0, d, T, bias=bias, vr=vr, **rk)
    valid = None if vr is None else (torch.arange(T, device=DEV)[None, :] < vr.long()[:, None])[..., None]
    check(what, y, ref, conv_bound(ref, mag, dtype), valid)
    if vr is not None:   # rows past each length: whole tiles beyond it are skipped (the sentinel stays); rows in a
        for b, n in enumerate(vr.tolist()):       # tile that straddles the end hold the zero-padded convolution (not checked)
            if n + 512 + (k - 1) * d < T and epi == "bias":
                assert (y[b, n + 512 + (k - 1) * d:] == 7.0).all(), (what, b)
    if controls:
        bound = conv_bound(ref, mag, dtype)
        tb = min(T - 2, 128 if T > 200 else T // 2)
        r_bad, _ = conv_ref(shifted_rows(x, tb), w, k, off0, d, T, bias=bias, vr=vr, **rk)
        must_fail(what, "input shifted by one row at a tile boundary", y, r_bad, bound, valid)
        r_bad, _ = conv_ref(x, perturbed_tap(w, k // 2, 2.0 ** -9), k, off0, d, T, bias=bias, vr=vr, **rk)
        must_fail(what, "one weight tap off by 2^-9 relative", y, r_bad, bound, valid)
        if N > 1:
            r_bad, _ = conv_ref(x, swapped_last(w), k, off0, d, T, bias=bias, vr=vr, **rk)
            must_fail(what, "two output channels of a 16-channel block exchanged", y, r_bad, bound, valid)
    return f


# every (k, d) of the AMP blocks at the narrow widths; T on both sides of each form's row tile (256 rows for the C = 24 / 48
# forms, 128 for C = 96); the first case of each family also runs the negative controls
NARROW = [(C, k, d) for C in (24, 48, 96) for k in (3, 7, 11) for d in (1, 3, 5)]


def narrow_expect(dtype, C, k, d, epi):
    t = "f16" if dtype == F16 else "bf16"
    if epi == "bias2_resid_acc":              # a per-batch bias takes the register-fed forms
        return {24: f"conv_narrow_taps<{t},1,2,{k},4,4>", 48: f"conv_narrow_taps<{t},2,3,{k},2,4>"}.get(C, f"gemm_conv<{t},2,2,4,3,2,64,persist>")
    if C == 24:
        return f"conv_narrow_lds<{t},24,{k},4,4,64>"
    if C == 48:
        return f"conv_narrow_lds<{t},48,{k},2,8,64>" if k == 11 else f"conv_narrow_lds<{t},48,{k},4,4,64>"
    if k == 3:
        return f"conv_narrow_lds<{t},96,3,1,8,64>"
    if k == 7:
        return f"conv_narrow_lds<{t},96,7,1,8,30>"
    return f"gemm_conv<{t},2,2,4,3,2,64,persist>"


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("C,k,d", NARROW)
def test_narrow_conv_fp64(nat, dtype, C, k, d):
    tile = 128 if C == 96 else 256
    for i, epi in enumerate(EPI_MATRIX):
        for T in (tile - 1, tile, tile + 1):
            run_conv(nat, dtype, 3, T, C, C, k, d, epi, seed=1000 + 7 * k + d + T, expect=narrow_expect(dtype, C, k, d, epi),
                     controls=(k == 7 and d == 3 and i in (0, 2) and T == tile + 1))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_c96_k7_halo_fills_the_row_tile_exactly(nat, dtype):
    """C = 96, 7 taps: the row tile is sized for a halo of 30 rows -- dilation 5 fills it exactly; dilation 6 (36 rows) must
    leave the LDS-staged form for the tiled kernel."""
    t = "f16" if dtype == F16 else "bf16"
    for T in (127, 128, 129, 1000):
        for epi in EPI_MATRIX[:3]:
            run_conv(nat, dtype, 2, T, 96, 96, 7, 5, epi, seed=2000 + T, expect=f"conv_narrow_lds<{t},96,7,1,8,30>",
                     controls=(T == 129 and epi == "resid_acc_third"))
            run_conv(nat, dtype, 2, T, 96, 96, 7, 6, epi, seed=2100 + T, expect=f"gemm_conv<{t},2,2,4,3,2,64,persist>")


# the wider vocoder stages (tiled kernel, 64- and 128-column tiles) at small T, with the production epilogues
WIDE = [(192, 3, 5), (192, 11, 1), (384, 7, 3), (768, 11, 5)]


@pytest.mark.parametrize("C,k,d", WIDE)
def test_wide_conv_fp64(nat, C, k, d):
    for i, epi in enumerate(("bias", "resid_third", "resid_acc_third")):
        run_conv(nat, F16, 2, 301, C, C, k, d, epi, seed=3000 + C + k, expect="gemm_conv<f16,*", controls=(i == 2 and C == 192))


RAGGED = [(24, 11, 5, 1100), (48, 7, 3, 900), (96, 7, 5, 700), (96, 3, 1, 700), (96, 11, 3, 700), (192, 7, 1, 600)]


@pytest.mark.parametrize("C,k,d,T", RAGGED)
def test_ragged_conv_fp64_each_element_at_its_own_length(nat, C, k, d, T):
    lens = [0, 1, 127, 128, 129, 255, 256, 257, T]
    vr = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for epi in ("bias", "resid", "resid_acc_third"):
        run_conv(nat, F16, len(lens), T, C, C, k, d, epi, seed=4000 + C + k, vr=vr, controls=(C == 48 and epi == "resid_acc_third"))


def convtr_as_conv(w, u):
    from indextts.BigVGAN.models import convtr_as_conv as f
    return f(w, u)


def run_upsampler(nat, dtype, B, Tn, cin, c, k, u, seed, expect=None, pin=True, controls=False, bias2=False):
    """ConvTranspose1d (stride u) as the vocoder launches it: 1 or 2 taps over [Tn (+1) rows][u*c columns], y_shift."""
    w = (rnd(cin, c, k, seed=seed) / math.sqrt(cin * k / u)).to(dtype)
    taps, off0, shift = convtr_as_conv(w, u)
    x = rnd(B, Tn, cin, seed=seed + 1).to(dtype)
    bias = (rnd(c, seed=seed + 2) * 0.1).float().repeat(u).contiguous()
    b2 = (rnd(B, u * c, seed=seed + 3) * 0.1).float() if bias2 else None
    Tu, N = Tn * u, u * c
    rows = Tn + 1 if taps.shape[0] == 2 else Tn
    y = torch.full((B, Tu, c), 7.0, dtype=dtype, device=DEV)
    nat.gemm_conv(dtype, B, Tn, rows, cin, N, nat.pack_weight(taps), x, y, taps=taps.shape[0], off0=off0, dil=1, bias=bias,
                  bias2=b2, y_bstride=Tu * c, y_shift=shift, y_limit=Tu * c)
    f = form(nat, expect, pin)

    def ref_of(tp):
        acc, mag = conv_ref(x, tp, tp.shape[0], off0, 1, rows, bias=bias, bias2=b2)
        return ups_slice(acc, shift, B, Tu, c), ups_slice(mag, shift, B, Tu, c)

    ref, mag = ref_of(taps)
    what = f"{f} upsampler B={B} Tn={Tn} {cin}->{c} k={k} u={u}"
    check(what, y, ref, conv_bound(ref, mag, dtype))
    if controls:
        tb = perturbed_tap(taps, taps.shape[0] - 1, 2.0 ** -9)
        must_fail(what, "one weight tap off by 2^-9 relative", y, ref_of(tb)[0], conv_bound(ref, mag, dtype))
    return f


# the six upsamplers of the vocoder: (Tn, cin, c, k, u)
UPS = [(37, 1536, 768, 8, 4), (60, 768, 384, 8, 4), (130, 384, 192, 4, 4), (257, 192, 96, 4, 4), (300, 96, 48, 4, 2),
       (515, 48, 24, 4, 2)]


@pytest.mark.parametrize("case", UPS)
def test_upsampler_fp64(nat, case):
    Tn, cin, c, k, u = case
    run_upsampler(nat, F16, 3, Tn, cin, c, k, u, seed=5000 + cin, controls=(cin == 48), bias2=(cin >= 768))


def test_pre_and_post_conv_fp64(nat):
    """conv_pre (1280 -> 1536, 7 taps, per-batch conditioning bias2) and conv_post (24 -> 1, 7 taps)."""
    B, T = 3, 141
    x = rnd(B, T, 1280, seed=6000).to(F16)
    w = (rnd(7, 1280, 1536, seed=6001) / math.sqrt(1280 * 7)).to(F16)
    bias, b2 = (rnd(1536, seed=6002) * 0.1).float(), (rnd(B, 1536, seed=6003) * 0.1).float()
    y = torch.empty(B, T, 1536, dtype=F16, device=DEV)
    nat.gemm_conv(F16, B, T, T, 1280, 1536, nat.pack_weight(w), x, y, taps=7, off0=-3, dil=1, bias=bias, bias2=b2)
    f = form(nat, "gemm_conv<f16,*")
    ref, mag = conv_ref(x, w, 7, -3, 1, T, bias=bias, bias2=b2)
    check(f"{f} conv_pre", y, ref, conv_bound(ref, mag, F16))
    for T in (255, 256, 257, 3001):
        run_conv(nat, F16, 3, T, 24, 1, 7, 1, "bias", seed=6100 + T, expect="conv_narrow<f16,1,1>", controls=(T == 257))


# ------------------------------------------------------------------------------------------------- activation
# act_ref, act_bound, EHW: tests/vocoder_refs.py


def run_act(nat, fir, dtype, B, T, C, seed, expect=None, lens=None, xscale=1.0, al=None, be=None, controls=False, pin=True,
            layout=0):
    up, dn = fir
    x = (rnd(B, T, C, seed=seed) * xscale).to(dtype)
    al = (rnd(C, seed=seed + 1) * 0.3).float() if al is None else al
    be = (rnd(C, seed=seed + 2) * 0.3).float() if be is None else be
    vr = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    if layout == 0:
        y = torch.full_like(x, 7.0)
        nat.aa_snake(x, al, be, up, dn, layout=0, out=y, valid_rows=vr)
    else:
        y = nat.aa_snake(x.transpose(1, 2).contiguous(), al, be, up, dn, layout=1).transpose(1, 2)
    f = form(nat, expect, pin)
    mfma = f.startswith("aa_snake_mfma")
    what = f"{f} B={B} T={T} C={C}" + ("" if lens is None else f" lens={lens}") + (f" |x|<={xscale}" if xscale != 1.0 else "")
    ref, e, ok = act_ref(x, al, be, up, dn, mfma, lens)
    bound = act_bound(ref, e, dtype)
    check(what, y, ref, bound, ok)
    if lens is not None:   # rows past each element's length are not written
        past = ~ok.expand_as(y)
        assert (y[past] == 7.0).all(), f"{what}: rows past a length were written"
    if controls:
        tb = 128 if T > 256 else T // 2
        must_fail(what, "input shifted by one row at a tile boundary", y, act_ref(shifted_rows(x, tb), al, be, up, dn, mfma, lens)[0], bound, ok)
        must_fail(what, "zero padding at the sequence end", y, act_ref(x, al, be, up, dn, mfma, lens, end_pad="zero")[0], bound, ok)
        dnb = perturbed_filter(dn, 2.0 ** -9)
        must_fail(what, "one down-filter tap off by 2^-9 relative", y, act_ref(x, al, be, up, dnb, mfma, lens)[0], bound, ok)
        if f.endswith("pair>"):     # two batch elements share a 48-channel slice: swap a channel across the pair
            xs = x.clone()
            xs[0, :, 5], xs[1, :, 5] = x[1, :, 5], x[0, :, 5]
            must_fail(what, "channel 5 of the two paired elements exchanged", y, act_ref(xs, al, be, up, dn, mfma, lens)[0], bound, ok)
        else:
            must_fail(what, "alpha and beta swapped", y, act_ref(x, be, al, up, dn, mfma, lens)[0], bound, ok)
            must_fail(what, "two channels of a 16-channel block exchanged", y, act_ref(swapped_last(x), al, be, up, dn, mfma, lens)[0], bound, ok)
    return f


def test_act_reference_matches_the_oracle(fir):
    """The explicit 12-tap form above is oracle.bigvgan_ref.activation1d (conv_transpose / conv1d form) in float64."""
    from oracle.bigvgan_ref import activation1d
    up, dn = fir
    x = rnd(2, 77, 8, seed=1)
    al, be = rnd(8, seed=2) * 0.3, rnd(8, seed=3) * 0.3
    ref, _, _ = act_ref(x, al, be, up, dn, False)
    o = activation1d(x.transpose(1, 2).cpu(), al.cpu(), be.cpu(), np.asarray(up, np.float64), np.asarray(dn, np.float64))
    assert (o.transpose(1, 2).to(DEV) - ref).abs().max().item() < 1e-12


def aa_tpw(nt, slices, C):
    """aa_tiles_per_wg (elementwise.hip): consecutive 128-row tiles one workgroup of the MFMA form walks."""
    t = (nt * slices) // (1536 if C > 96 else 3072)
    return max(1, min(8, t))


# (B, T, C, expected form): MFMA forms at C = 24..192 (the switch is B*T >= 32768), C = 24 paired / odd / ragged, T not a
# multiple of the 128-row tile, several tiles per workgroup with a tile count the workgroup count does not divide
ACT_MFMA = [
    (1, 32768, 48, "aa_snake_mfma<3>"), (1, 32767, 48, "aa_snake_btc<f16,48>"),
    (1, 32768, 24, "aa_snake_mfma<2>"), (1, 32767, 24, "aa_snake_btc<f16,24>"),
    (2, 16384, 24, "aa_snake_mfma<3,pair>"), (2, 16383, 24, "aa_snake_btc<f16,24>"),
    (8, 4100, 96, "aa_snake_mfma<3>"), (8, 4100, 192, "aa_snake_mfma<3>"), (3, 11001, 24, "aa_snake_mfma<2>"),
    (4, 8200, 24, "aa_snake_mfma<3,pair>"),
    (32, 8400, 192, "aa_snake_mfma<3>"),      # 66 tiles x 4 slices x 32: 5 tiles per workgroup, 66 % 5 = 1
    (24, 32800, 48, "aa_snake_mfma<3>"),      # 257 tiles: 2 per workgroup, odd count
    (64, 24650, 24, "aa_snake_mfma<3,pair>"),  # 193 tiles x 32 pairs: 2 per workgroup
]


@pytest.mark.parametrize("B,T,C,expect", ACT_MFMA)
def test_act_fp16_forms_fp64(nat, fir, B, T, C, expect):
    if T >= 8400 and B >= 24:     # several tiles per workgroup, a tile count the tiles per workgroup do not divide
        nt = (T + 127) // 128
        slices = B // 2 if expect.endswith("pair>") else (C // 48) * B
        tpw = aa_tpw(nt, slices, C)
        assert tpw > 1 and nt % tpw != 0, (nt, tpw)
    run_act(nat, fir, F16, B, T, C, seed=7000 + C + B, expect=expect,
            controls=(B, T) in ((1, 32768), (2, 16384), (1, 32767)))


@pytest.mark.parametrize("T", [1, 2, 5, 11, 12, 13])
def test_act_fp16_short_sequences_mfma(nat, fir, T):
    B = (32768 + T - 1) // T
    B += B % 2
    run_act(nat, fir, F16, B, T, 48, seed=7100 + T, expect="aa_snake_mfma<3>")
    run_act(nat, fir, F16, B, T, 24, seed=7200 + T, expect="aa_snake_mfma<3,pair>")
    run_act(nat, fir, F16, B + 1, T, 24, seed=7300 + T, expect="aa_snake_mfma<2>")


@pytest.mark.parametrize("C,expect", [(48, "aa_snake_mfma<3>"), (24, "aa_snake_mfma<2>"), (192, "aa_snake_mfma<3>")])
def test_act_fp16_ragged_mfma(nat, fir, C, expect):
    T = 4000
    lens = [0, 1, 127, 128, 129, 255, 256, 257, 3999, T]
    run_act(nat, fir, F16, len(lens), T, C, seed=7400 + C, lens=lens, expect=expect, controls=(C == 24))


@pytest.mark.parametrize("dtype,C", [(F16, 384), (F16, 768), (BF16, 24), (BF16, 48), (BF16, 96), (BF16, 192), (BF16, 384),
                                     (BF16, 768), (F16, 32), (BF16, 32)])
def test_act_valu_forms_fp64(nat, fir, dtype, C):
    t = "f16" if dtype == F16 else "bf16"
    cs = 64 if C % 64 == 0 else 48 if C % 48 == 0 else 32 if C % 32 == 0 else 24
    B, T = (8, 4500) if C >= 384 or dtype == BF16 else (8, 4000)
    run_act(nat, fir, dtype, B, T, C, seed=7500 + C, expect=f"aa_snake_btc<{t},{cs}>", controls=(C in (384, 48)))
    T = 3200                 # (10 x 3 200 rows: below the MFMA form's switch also for fp16 at C <= 192)
    lens = [0, 1, 75, 76, 77, 159, 160, 161, T - 1, T]
    run_act(nat, fir, dtype, len(lens), T, C, seed=7600 + C, lens=lens, expect=f"aa_snake_btc<{t},{cs}>")


@pytest.mark.parametrize("dtype,C,B,T,expect", [(F16, 48, 1, 32768, "aa_snake_mfma<3>"), (F16, 24, 2, 16384, "aa_snake_mfma<3,pair>"),
                                                (F16, 384, 2, 3000, "aa_snake_btc<f16,64>"), (F16, 48, 2, 3000, "aa_snake_btc<f16,48>"),
                                                (BF16, 48, 2, 3000, "aa_snake_btc<bf16,48>")])
def test_act_large_arguments(nat, fir, dtype, C, B, T, expect):
    """|u e^alpha| up to ~2 000 rad (~320 revolutions: past the +-256 of the hardware sine's documented input range).  The
    16-bit VALU form feeds v_sin_f32 unreduced; on MI355X it stays within the bound there, so aa_sin needs no reduction."""
    al = torch.full((C,), 0.5, device=DEV)
    run_act(nat, fir, dtype, B, T, C, seed=7700 + C, xscale=300.0, al=al, expect=expect)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("B,C,T", [(2, 24, 3001), (3, 48, 1000), (1, 96, 257)])
def test_act_layout1_fp64(nat, fir, dtype, B, C, T):
    t = "f16" if dtype == F16 else "bf16"
    run_act(nat, fir, dtype, B, T, C, seed=7800 + T, expect=f"aa_snake_bct<{t}>", layout=1, controls=(C == 48))


# ------------------------------------------------------------------------------------------------- production forward
@pytest.fixture(scope="module")
def production(nat):
    """Signatures and forms of one eager fp16 BigVGAN.forward at production geometry (batch 32, 140 latent frames)."""
    from indextts.BigVGAN.models import BigVGAN
    from indextts.utils.config import Config
    v = BigVGAN(Config(weights.reference_config()["bigvgan"]))
    v.load_state_dict(weights.bigvgan_state_dict())
    v.to(DEV).to(F16).remove_weight_norm()
    B, Tn = 32, 140
    lat = rnd(B, Tn, 1280, seed=9000).float()
    spk = rnd(B, 1, 512, seed=9001).float() * 0.1
    rec = []
    g0, a0 = nat.gemm_conv, nat.aa_snake

    def g(dtype, B, Tin, Tout, Cin, N, wp, x, y, **kw):
        g0(dtype, B, Tin, Tout, Cin, N, wp, x, y, **kw)
        rec.append(("conv", dtype, B, Tin, Tout, Cin, N, kw.get("taps", 1), kw.get("off0", 0), kw.get("dil", 1),
                    kw.get("bias") is not None, kw.get("bias2") is not None, kw.get("resid") is not None,
                    bool(kw.get("accumulate", False)), float(kw.get("scale", 1.0)), int(kw.get("y_shift", 0)),
                    y.shape[-1], nat.last_kernel()))

    def a(x, al, be, up, dn, layout=0, out=None, valid_rows=None):
        y = a0(x, al, be, up, dn, layout=layout, out=out, valid_rows=valid_rows)
        rec.append(("act", x.dtype, x.shape[0], x.shape[1], x.shape[2], nat.last_kernel()))
        return y

    nat.gemm_conv, nat.aa_snake = g, a
    try:
        with torch.no_grad():
            v(lat, speaker_embedding=spk)
        torch.cuda.synchronize()
    finally:
        nat.gemm_conv, nat.aa_snake = g0, a0
    del v
    return rec


def test_production_signatures_fp64(nat, fir, production):
    """Every distinct (C_in, N, taps, dilation, epilogue, form) of the forward, at the same batch and a T of at most 1 200
    rows (the same form: asserted), against the fp64 reference."""
    seen = set()
    for i, r in enumerate(production):
        if r[0] == "act":
            _, dtype, B, T, C, f = r
            key = ("act", C, f)
            if key in seen:
                continue
            seen.add(key)
            Tc = min(T, max(1200, (32768 + B - 1) // B))
            run_act(nat, fir, dtype, B, Tc, C, seed=9100 + i, expect=f, pin=False)
            continue
        (_, dtype, B, Tin, Tout, Cin, N, taps, off0, dil, has_b, has_b2, has_r, acc, scale, y_shift, c, f) = r
        key = (Cin, N, taps, dil, off0, has_b2, has_r, acc, scale, y_shift, f)
        if key in seen:
            continue
        seen.add(key)
        if c != N:                               # an upsampler: [Tin (+1) rows][u*c] stored shifted into [u*Tin][c]
            u = N // c
            k = 2 * u if taps == 2 else u
            assert Tout == Tin + (taps - 1) and y_shift == -((k - u) // 2) * c, r
            run_upsampler(nat, dtype, B, min(Tin, 150), Cin, c, k, u, seed=9200 + i, expect=f, pin=False, bias2=has_b2)
            continue
        T = min(Tin, 1200)
        if has_b2:      # conv_pre: the conditioning bias, no residual
            x = rnd(B, T, Cin, seed=9300 + i).to(dtype)
            w = (rnd(taps, Cin, N, seed=9301 + i) / math.sqrt(Cin * taps)).to(dtype)
            bias, b2 = (rnd(N, seed=9302) * 0.1).float(), (rnd(B, N, seed=9303) * 0.1).float()
            y = torch.empty(B, T, N, dtype=dtype, device=DEV)
            nat.gemm_conv(dtype, B, T, T, Cin, N, nat.pack_weight(w), x, y, taps=taps, off0=off0, dil=dil, bias=bias, bias2=b2)
            form(nat, f, pin=False)
            ref, mag = conv_ref(x, w, taps, off0, dil, T, bias=bias, bias2=b2)
            check(f"{f} conv_pre", y, ref, conv_bound(ref, mag, dtype))
            continue
        epi = [e for e, v in EPIS.items() if v == (has_r, acc, scale if scale == 1.0 else 1.0 / 3.0, False)]
        assert len(epi) == 1 and abs(scale - EPIS[epi[0]][2]) < 1e-7 and off0 == -((taps - 1) * dil // 2), r
        run_conv(nat, dtype, B, T, Cin, N, taps, dil, epi[0], seed=9400 + i, expect=f, pin=False)
    assert len(seen) >= 20


def test_production_forms_are_pinned(nat, production):
    """Every kernel form the production forward launched is pinned by the edge matrix of this file (which must have run
    first, as it does in file order): a change to the dispatch code that adds a form no case pins fails here."""
    used = sorted({r[-1] for r in production})
    print("kernel forms of the production forward:", ", ".join(used))
    assert any(f.startswith("aa_snake_mfma<") for f in used) and any(f.startswith("conv_narrow_lds<") for f in used), used
    missing = [f for f in used if f not in PINNED]
    assert not missing, f"forms of the production forward no edge case pins: {missing} (used: {used})"
