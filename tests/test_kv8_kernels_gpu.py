"""The two FP8 KV cache kernels through the C ABI (include/indextts_hip.h), bf16 and f16.

itts_kv8_store: the codes it writes equal the host quantiser's (indextts/utils/quant.py) bit for bit, and every other byte of the
pool keeps its sentinel.

itts_attn_decode_kv8 against float64 attention over the DECODED pool plus the DECODED new key: the operands are identical, so the
bound is the one of the 16-bit decode attention (test_decode_kernels_gpu.py, "Decode attention"):
      bound = ulp_T(ref) + C_ATTN A,   C_ATTN = 2^-16,   A = sum_j p_j |v_j|  (v_j scaled: what the output is a mean of).
The fp32-level budget is that kernel's: a score is 16 fmaf per lane and 2 shuffle additions here (8 and 3 there), the sums take
at most 17 additions per lane and 6 merge steps; both scales are powers of two and cost no rounding.
Negative controls (`bad`): the new key left out, v_scale ignored, the mask off by one at pad_b (either way).
After the launch the codes at *pos equal the host quantiser of the new k / v, the skipped row's blocks and every other byte are
unchanged.  P = kv8_refs.P_FIRST = 256 keys is the full pass; the sized arms end at 64 / 128 / 192 / 256 key slots from pad & ~15.
"""
import numpy as np
import pytest
import torch

import kv8_refs as R
from fp64_check import bad, ok, tname, ulp
from indextts.utils import quant

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
C_ATTN = 2.0 ** -16
SENT = 0x5A


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- store
@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("form", ["padded", "packed"])
def test_kv8_store_writes_the_host_quantisers_codes_and_nothing_else(nat, dtype, bs, form):
    H, D = 3, 3 * 64
    scale = torch.tensor([[2.0 ** -3, 1.0, 2.0 ** 2], [2.0 ** 1, 2.0 ** -5, 1.0]], dtype=torch.float32, device=DEV)   # [K | V][H]
    if form == "padded":
        B, S, pads = 3, 37, [0, 5, 36]
        rows = [(b * S + s, b, s) for b in range(B) for s in range(pads[b], S)]          # (qkv row, table row, position)
        spans = [(0, S - 1)] * B
        M = B * S
    else:
        lens, shift = [1, 16, 33], [40, 7, 15]
        B, S = 3, max(lens)
        off = np.concatenate([[0], np.cumsum(lens)])
        rows = [(int(off[b]) + s, b, shift[b] + s) for b in range(B) for s in range(lens[b])]
        spans = [(shift[b], shift[b] + lens[b] - 1) for b in range(B)]
        M = int(off[-1])
    qkv = (R.rnd(M, 3, H, 64, seed=bs + len(form), device=DEV) * 1.5).to(dtype)
    qkv[0, 1, 0, :4] = torch.tensor([1000.0, -1000.0, 56.0, -56.01], dtype=dtype)        # saturates at scale 2^-3; 448 exactly; just past it
    tab, blocks = R.ring_table(spans, bs, seed=3)
    kc = torch.full((blocks, H, bs, 64), SENT, dtype=torch.uint8, device=DEV)
    vc = torch.full_like(kc, SENT)
    want_k, want_v = kc.clone(), vc.clone()
    for r, b, p in rows:
        R.scatter(want_k, tab, bs, b, [p], quant.quantize_kv_e4m3(qkv[r, 1], scale[0][:, None])[:, None])
        R.scatter(want_v, tab, bs, b, [p], quant.quantize_kv_e4m3(qkv[r, 2], scale[1][:, None])[:, None])
    flat = qkv.view(M, 3 * D).contiguous()
    if form == "padded":
        nat.kv8_store(flat, kc, vc, scale, B, S, H, pad=i32(pads), kv_tab=i32(tab), kv_bs=bs)
    else:
        nat.kv8_store(flat, kc, vc, scale, B, S, H, row_off=i32(off), cache_shift=i32(shift), kv_tab=i32(tab), kv_bs=bs)
    torch.cuda.synchronize()
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)
    assert int((want_k != SENT).sum()) > 0 and not ((kc & 0x7F) == 0x7F).any()


# ---------------------------------------------------------------------------------------------------------------- attention
def arm_pads(pos, r):
    """pads whose key slots pos - (pad & ~15) are 64 / 128 / 192 / 256 plus pos % 16, r positions into their group"""
    return [((pos - n) & ~15) + r for n in (64, 128, 192, 256)]


LAUNCHES = [
    # (pos, bs, pads, packed output)
    (304, 16, arm_pads(304, 0) + arm_pads(304, 3) + [304, 304 - 14, 304 - 15, 304 - 16, 304 - 255, 304 - 256, 0, 21], False),
    (305, 16, arm_pads(305, 0) + arm_pads(305, 5) + [305, 305 - 14, 305 - 15, 305 - 16, 305 - 255, 305 - 256, 0, 44], True),
    (304, 32, arm_pads(304, 7) + [304, 304 - 15, 304 - 16, 304 - 255, 0, 77], True),
    (305, 64, arm_pads(305, 9) + [305, 305 - 15, 305 - 16, 305 - 256, 0, 130], False),
    (64 * 16 + 41, 16, [1065 - 700, 1065 - 30, 1065, 1065 - 259, 200, 1065 - 16, 1000], False),   # positions past 64 * bs: the ring wraps
]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
@pytest.mark.parametrize("launch", range(len(LAUNCHES)))
def test_attn_decode_kv8_fp64(nat, dtype, launch):
    """Rows of one launch: both sides of every sized arm's limit (slots 64 / 65 ... 256 / 257 over launches 0-3, pads on and off a
    multiple of 16), one key (pos = pad), 15 / 16 / 17 keys, P and P + 1 keys, a full row, and a skipped last row."""
    pos, bs, pads, packed = LAUNCHES[launch]
    H, B = 2, len(pads)
    skip_row = B - 1
    k_scale, v_scale = torch.tensor([2.0 ** -3, 1.0]), torch.tensor([2.0 ** 2, 1.0])
    q, kn, vn, kcodes, vcodes = R.decode_case(dtype, pads, pos, H, k_scale, v_scale, seed=900 + launch, device=DEV)
    spans = [(p, pos) for p in pads]
    tab, blocks = R.ring_table(spans, bs, seed=launch)
    g = torch.Generator().manual_seed(launch)
    fill = lambda: quant.quantize_kv_e4m3(torch.randn(blocks, H, bs, 64, generator=g), 0.25).to(DEV)   # noqa: E731  finite stale codes
    kc, vc = fill(), fill()
    for b, p in enumerate(pads):
        span = list(range(p // bs * bs, pos + 1))
        R.scatter(kc, tab, bs, b, span, kcodes[b][:, span[0]:])
        R.scatter(vc, tab, bs, b, span, vcodes[b][:, span[0]:])
    kc0, vc0 = kc.clone(), vc.clone()
    qkv = torch.stack([q, kn, vn], 1).reshape(B, 3 * H * 64).contiguous()
    scale = torch.stack([k_scale, v_scale]).to(DEV, torch.float32).contiguous()
    skip = torch.zeros(B, dtype=torch.int32, device=DEV)
    skip[skip_row] = 1
    out = torch.full(((B + 15) // 16 * 16 * H * 64,) if packed else (B, H * 64), 7.0, dtype=dtype, device=DEV)
    nat.attn_decode_kv8(qkv, kc, vc, out, i32(pads), i32([pos]), scale, B, H, out_packed=packed, skip_rows=skip, kv_tab=i32(tab), kv_bs=bs)
    torch.cuda.synchronize()
    got = nat.unpack_activation(out, B, H * 64) if packed else out
    what = f"attn_decode_kv8 {tname(dtype)} bs={bs} pos={pos} pads={pads} {'packed' if packed else 'row-major'}"
    assert (got[skip_row] == 7.0).all(), f"{what}: the skipped row was written"

    # the append: codes at *pos = the host quantiser of the new k / v; the skipped row's blocks and every other byte unchanged
    ksd, vsd = k_scale.to(DEV)[None, :, None], v_scale.to(DEV)[None, :, None]
    kn_c, vn_c = quant.quantize_kv_e4m3(kn, ksd), quant.quantize_kv_e4m3(vn, vsd)
    want_k, want_v = kc0.clone(), vc0.clone()
    for b in range(B):
        if b != skip_row:
            R.scatter(want_k, tab, bs, b, [pos], kn_c[b][:, None])
            R.scatter(want_v, tab, bs, b, [pos], vn_c[b][:, None])
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v), f"{what}: the pool after the launch"
    assert not torch.equal(kc, kc0)

    # fp64 attention over the decoded pool plus the decoded new key
    qd = q.double()
    kd, vd = quant.dequantize_kv(kcodes, ksd[..., None]), quant.decode_e4m3(vcodes)       # (v's scale multiplies the result)
    knd, vnd = quant.dequantize_kv(kn_c, ksd), quant.decode_e4m3(vn_c)
    valid = torch.ones(B, 1, dtype=torch.bool, device=DEV)
    valid[skip_row] = False
    ref, A = R.attention(qd, kd, vd, knd, vnd, pads, pos, v_scale)
    bound = ulp(ref, dtype) + C_ATTN * A
    ok(what, got, ref, bound, valid)
    if launch not in (1, 4):
        return

    def dbad(control, r):      # a control that leaves a row without any key says nothing about that row
        fin = torch.isfinite(r).all(1, keepdim=True)
        bad(what, control, got, torch.nan_to_num(r), bound, valid & fin)
    dbad("the new key left out", R.attention(qd, kd, vd, knd, vnd, pads, pos, v_scale, new_key=False)[0])
    dbad("the new key taken unquantised", R.attention(qd, kd, vd, kn.double(), vn.double() / vsd, pads, pos, v_scale)[0])
    dbad("v_scale ignored", R.attention(qd, kd, vd, knd, vnd, pads, pos, torch.ones(H))[0])
    dbad("k_scale ignored", R.attention(qd, quant.decode_e4m3(kcodes), vd, quant.decode_e4m3(kn_c), vnd, pads, pos, v_scale)[0])
    dbad("the key at pad[b] left out", R.attention(qd, kd, vd, knd, vnd, pads, pos, v_scale, lo_shift=1)[0])
    dbad("the key at pad[b] - 1 let in", R.attention(qd, kd, vd, knd, vnd, pads, pos, v_scale, lo_shift=-1)[0])


def test_kv8_entry_points_refuse_and_launch_nothing(nat):
    """fp32, a bad kv_bs and null pointers: an error each, and the buffers keep their bytes."""
    B, H, bs = 2, 2, 16
    tab, blocks = R.ring_table([(0, 20)] * B, bs, seed=1)
    kc = torch.full((blocks, H, bs, 64), SENT, dtype=torch.uint8, device=DEV)
    vc = kc.clone()
    scale = torch.ones(2, H, device=DEV)
    out = torch.full((B, H * 64), 7.0, dtype=BF16, device=DEV)
    pad, pos, tabd = i32([0, 3]), i32([17]), i32(tab)
    qkv = torch.ones(B, 3 * H * 64, dtype=BF16, device=DEV)
    for kw, word in ((dict(qkv=qkv.float()), "bf16 / f16"), (dict(kv_bs=48), "kv_bs"), (dict(kv_bs=8), "kv_bs"), (dict(kv_tab=None), "null"),
                     (dict(kv_scale=None), "null"), (dict(pos=None), "null")):
        a = dict(qkv=qkv, kcache=kc, vcache=vc, out=out, pad=pad, pos=pos, kv_scale=scale, kv_tab=tabd, kv_bs=bs)
        a.update(kw)
        with pytest.raises(nat.NativeError, match=word):
            nat.attn_decode_kv8(a["qkv"], a["kcache"], a["vcache"], a["out"] if a["qkv"].dtype == BF16 else out.float(), a["pad"], a["pos"],
                                a["kv_scale"], B, H, kv_tab=a["kv_tab"], kv_bs=a["kv_bs"])
    for kw, word in ((dict(qkv=qkv.float()), "bf16 / f16"), (dict(kv_bs=0), "kv_bs"), (dict(kv_tab=None), "null")):
        a = dict(qkv=qkv, kv_tab=tabd, kv_bs=bs)
        a.update(kw)
        with pytest.raises(nat.NativeError, match=word):
            nat.kv8_store(a["qkv"], kc, vc, scale, B, 1, H, kv_tab=a["kv_tab"], kv_bs=a["kv_bs"])
    torch.cuda.synchronize()
    assert (kc == SENT).all() and (vc == SENT).all() and (out == 7.0).all()
