"""The segmented forms of the three sequence-mixing front-end kernels (include/indextts_hip.h) against the single-prompt
entry points they share their bodies with: every segment's output is BIT-identical to the single-prompt call on that segment
alone.  The single-prompt forms are pinned to fp64 by test_frontend_kernels_gpu.py, so no tolerance appears here.

Shapes: t_p in {1, 5, 16, 17, 33, 59} in one call -- 5 is shorter than the half-width of the 15 depthwise taps, 16 and 17 straddle
a row tile, 33 is more than one 16-query tile and more than one 32-key step -- with the segment order shuffled against the length
order.  Outputs are filled with a sentinel (rows outside every segment must keep it), padding rows of the inputs hold 1000 (a
kernel that read one as data would not reproduce the single-prompt bits)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS = [17, 1, 59, 5, 33, 16]
SENT = -7.0
DTYPES = [torch.float16, torch.bfloat16]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def space_of(lens, odd=True):
    from indextts.gpt.conditioner import prompt_row_space
    # 2 t + 1 frames give t rows; so do 2 t + 2 (the last frame is then outside every window)
    return prompt_row_space([2 * t + 1 + (0 if odd or i % 2 else 1) for i, t in enumerate(lens)])


def rows_with_padding(sp, cols, seed, dtype, scale=1.0):
    """[M, cols] of the row space: random rows inside the segments, 1000 on the padding rows"""
    x = torch.full((sp["M"], cols), 1000.0, device=DEV)
    for i, (r0, t) in enumerate(zip(sp["row0"], sp["t"])):
        x[r0:r0 + t] = rnd(t, cols, seed=seed + i, scale=scale)
    return x.to(dtype)


def outside(sp, rows):
    keep = torch.ones(rows, dtype=torch.bool)
    for r0, t in zip(sp["row0"], sp["t"]):
        keep[r0:r0 + t] = False
    return keep.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Fq,Cn", [(20, 64), (5, 8)])           # the staged (LDS) and the direct store form
@pytest.mark.parametrize("lens", [LENS, [33]])
def test_subsample_conv_seg_equals_each_prompt_alone(dtype, Fq, Cn, lens):
    from indextts import _native as nat
    from indextts.gpt.conditioner import prompt_seg_records
    sp = space_of(lens, odd=False)
    f2 = (Fq - 3) // 2 + 1
    mel = rnd(sp["total_frames"], Fq, seed=1, scale=2.0)
    w, b = rnd(Cn, 9, seed=2, scale=0.3), rnd(Cn, seed=3, scale=0.1)
    recs, ntiles = prompt_seg_records(sp, 32)["conv"]
    y = torch.full((sp["M"], Cn * f2), SENT, dtype=dtype, device=DEV)
    nat.subsample_conv_seg(mel, w, b, y, nat.SegTable(recs, ntiles, DEV))
    for r0, t, f0, T in zip(sp["row0"], sp["t"], sp["frame0"], sp["frames"]):
        one = torch.full((t, Cn * f2), SENT, dtype=dtype, device=DEV)
        nat.subsample_conv(mel[f0:f0 + T].contiguous(), w, b, one)
        assert torch.equal(y[r0:r0 + t], one), (r0, t)
    assert (y[outside(sp, sp["M"])] == SENT).all() and not (y[:1] == SENT).all()
    if len(lens) == 1:                                # N = 1: the old entry point over the whole output
        old = torch.full_like(y, SENT)
        nat.subsample_conv(mel, w, b, old)
        assert torch.equal(y, old)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lens", [LENS, [33]])
def test_mha_small_seg_conformer_geometry(dtype, lens):
    """Queries = keys = the segment's rows, relative-position term with a table built for the longest segment."""
    from indextts import _native as nat
    from indextts.gpt.conditioner import prompt_seg_records
    H = 2
    d = H * 64
    sp = space_of(lens)
    M, tmax = sp["M"], max(sp["t"])
    qkv = rows_with_padding(sp, 3 * d, 10, dtype, 0.7)
    pos = (rnd(H, tmax, 64, seed=6) * 0.5).to(dtype)
    u, vb = rnd(d, seed=7) * 0.2, rnd(d, seed=8) * 0.2
    recs, ntiles = prompt_seg_records(sp, 32)["enc"]
    out = torch.full((M * d,), SENT, dtype=dtype, device=DEV)
    nat.mha_small_seg(qkv, qkv[:, d:], qkv[:, 2 * d:], out, M, M, H, 3 * d, 3 * d, 3 * d, M // 16, 0.125, nat.SegTable(recs, ntiles, DEV),
                      pos=pos, bias_u=u, bias_v=vb, pos_tk=tmax)
    got = nat.unpack_activation(out, M, d)
    for r0, t in zip(sp["row0"], sp["t"]):
        mtp = (t + 15) // 16
        one = torch.full((mtp * 16 * d,), SENT, dtype=dtype, device=DEV)
        seg = qkv[r0:r0 + t]
        nat.mha_small(seg, seg[:, d:], seg[:, 2 * d:], one, t, t, H, 3 * d, 3 * d, 3 * d, mtp, 0.125, pos=pos[:, :t].contiguous(),
                      bias_u=u, bias_v=vb)
        assert torch.equal(got[r0:r0 + t], nat.unpack_activation(one, t, d)), (r0, t)
        assert torch.isfinite(got[r0:r0 + t].float()).all()
    assert (got[outside(sp, M)] == SENT).all()
    if len(lens) == 1:
        old = torch.full_like(out, SENT)
        nat.mha_small(qkv, qkv[:, d:], qkv[:, 2 * d:], old, lens[0], lens[0], H, 3 * d, 3 * d, 3 * d, M // 16, 0.125, pos=pos, bias_u=u,
                      bias_v=vb)
        assert torch.equal(out, old)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mha_small_seg_perceiver_geometry(dtype):
    """Tq = 32 latent rows per segment, two key ranges: the segment's latent rows, then its context rows behind ALL latent rows."""
    from indextts import _native as nat
    from indextts.gpt.conditioner import prompt_seg_records
    H, NL = 2, 32
    d = H * 64
    sp = space_of(LENS)
    n, M = len(LENS), sp["M"]
    rl, ra = n * NL, n * NL + sp["M"]
    qkv = torch.cat([rnd(rl, 3 * d, seed=20, scale=0.7).to(dtype), rows_with_padding(sp, 3 * d, 30, dtype, 0.7)], 0)
    recs, ntiles = prompt_seg_records(sp, NL)["per"]
    out = torch.full((rl * d,), SENT, dtype=dtype, device=DEV)
    nat.mha_small_seg(qkv, qkv[:, d:], qkv[:, 2 * d:], out, rl, ra, H, 3 * d, 3 * d, 3 * d, rl // 16, 0.125, nat.SegTable(recs, ntiles, DEV))
    got = nat.unpack_activation(out, rl, d)
    for p, (r0, t) in enumerate(zip(sp["row0"], sp["t"])):
        alone = torch.cat([qkv[p * NL:(p + 1) * NL], qkv[rl + r0:rl + r0 + t]], 0).contiguous()     # [latents ; context] of this prompt
        one = torch.full((NL * d,), SENT, dtype=dtype, device=DEV)
        nat.mha_small(alone, alone[:, d:], alone[:, 2 * d:], one, NL, NL + t, H, 3 * d, 3 * d, 3 * d, NL // 16, 0.125)
        assert torch.equal(got[p * NL:(p + 1) * NL], nat.unpack_activation(one, NL, d)), (p, t)
    assert torch.isfinite(got.float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps", [15, 7, 31])
@pytest.mark.parametrize("lens", [LENS, [33]])
def test_glu_dwconv_ln_silu_seg_equals_each_segment_alone(dtype, taps, lens):
    from indextts import _native as nat
    from indextts.gpt.conditioner import prompt_seg_records
    Cn = 128
    sp = space_of(lens)
    M = sp["M"]
    x = rows_with_padding(sp, 2 * Cn, 40, dtype)
    w, b = rnd(Cn, taps, seed=10, scale=0.3), rnd(Cn, seed=11, scale=0.1)
    lw, lb = 1.0 + rnd(Cn, seed=12, scale=0.1), rnd(Cn, seed=13, scale=0.1)
    recs, ntiles = prompt_seg_records(sp, 32)["enc"]
    y = torch.full((M * Cn,), SENT, dtype=dtype, device=DEV)
    nat.glu_dwconv_ln_silu_seg(x, w, b, lw, lb, y, Cn, M // 16, nat.SegTable(recs, ntiles, DEV))
    got = nat.unpack_activation(y, M, Cn)
    for r0, t in zip(sp["row0"], sp["t"]):
        mtp = (t + 15) // 16
        one = torch.full((mtp * 16 * Cn,), SENT, dtype=dtype, device=DEV)
        nat.glu_dwconv_ln_silu(x[r0:r0 + t], w, b, lw, lb, one, t, Cn, mtp)
        assert torch.equal(got[r0:r0 + t], nat.unpack_activation(one, t, Cn)), (r0, t)
        assert torch.isfinite(got[r0:r0 + t].float()).all()
    assert (got[outside(sp, M)] == SENT).all()
    if len(lens) == 1:
        old = torch.full_like(y, SENT)
        nat.glu_dwconv_ln_silu(x, w, b, lw, lb, old, lens[0], Cn, M // 16)
        assert torch.equal(y, old)


BAD_TABLES = {
    "row0 not a multiple of 16": ([(0, 5, 0, 11), (24, 5, 11, 11)], None),
    "overlapping segments": ([(0, 20, 0, 41), (16, 5, 41, 11)], None),
    "zero length": ([(0, 5, 0, 11), (16, 0, 11, 3)], None),
    "tile map against the records": ([(0, 5, 0, 11), (16, 5, 11, 11)], [0, 0, -1]),
}


@pytest.mark.parametrize("why", sorted(BAD_TABLES))
def test_invalid_tables_are_refused_and_launch_nothing(why):
    from indextts import _native as nat
    recs, tmap = BAD_TABLES[why]
    dtype, Cn, Fq, H = torch.float16, 128, 5, 2
    tab = nat.SegTable(recs, 3, DEV, tile_map=tmap)
    M = 48
    mel, w9, b9 = rnd(64, Fq, seed=1), rnd(8, 9, seed=2), rnd(8, seed=3)
    y0 = torch.full((M, 8 * 2), SENT, dtype=dtype, device=DEV)
    with pytest.raises(nat.NativeError, match=r"code 1"):
        nat.subsample_conv_seg(mel, w9, b9, y0, tab)
    # the same rows as an attention / convolution-module table (words 2.. = key rows / unused)
    enc = nat.SegTable([(r[0], r[1], r[0], max(r[1], 1), 0, 0, r[0] // 16 * 16) for r in recs], 3, DEV, tile_map=tmap)
    qkv = rnd(M, 3 * H * 64, seed=4).to(dtype)
    y1 = torch.full((M * H * 64,), SENT, dtype=dtype, device=DEV)
    with pytest.raises(nat.NativeError, match=r"code 1"):
        nat.mha_small_seg(qkv, qkv[:, H * 64:], qkv[:, 2 * H * 64:], y1, M, M, H, 3 * H * 64, 3 * H * 64, 3 * H * 64, 3, 0.125, enc)
    x = rnd(M, 2 * Cn, seed=5).to(dtype)
    y2 = torch.full((M * Cn,), SENT, dtype=dtype, device=DEV)
    with pytest.raises(nat.NativeError, match=r"code 1"):
        nat.glu_dwconv_ln_silu_seg(x, rnd(Cn, 15, seed=6), rnd(Cn, seed=7), rnd(Cn, seed=8), rnd(Cn, seed=9), y2, Cn, 3, enc)
    torch.cuda.synchronize()
    assert (y0 == SENT).all() and (y1 == SENT).all() and (y2 == SENT).all()
    assert C.sizeof(nat.SegTableArgs) == 24
