"""ittv_delta_project (csrc/delta.hip, include/indextts_voice.h) against float64, through indextts._native_voice:
Y = op(D) X with D = float(Wt) - float(Wb), both op forms, the storage pairs (Wt, Wb) = (fp16, fp16), (bf16, fp16), (fp32, bf16).

Shapes (K, N, c): (16, 16, 16) one tile, one half-used 32-wide step; (48, 80, 32) N = 2.5 steps, no split; (272, 144, 80) the widest
c, K and N no multiples of 32 / 128 (a partial column tile in the transposed form) and a split reduction in both forms whose last
piece is shorter; (1280, 3840, 32) the real attn.c_attn, 12 and 16 pieces.

Bound, per element: the standard fp32 dot-product bound (L + 2) 2^-24 sum |D| |X| over the reduction length L -- L roundings of
the fmaf chain (a split chain has fewer per piece plus one per piece joined), one for D where an operand is fp32 (the difference
of two 16-bit values is exact), one to spare.  Control: the same check against a reference whose Wb was first rounded to bf16 must
fail -- on the pairs whose Wb is fp16; in the third pair Wb IS bf16, that rounding changes nothing and there is nothing to refuse.
Two launches on the same inputs give the same bits; K = 24 is refused, nothing is launched.
`-s` prints the `fp64 | kind | case | ratio` lines of profiles/voice_extract_fp64.txt."""
import pytest
import torch

from fp64_check import bad, ok, rnd, tname

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(16, 16, 16), (48, 80, 32), (272, 144, 80), (1280, 3840, 32)]
PAIRS = [(torch.float16, torch.float16), (torch.bfloat16, torch.float16), (torch.float32, torch.bfloat16)]


@pytest.fixture(scope="module")
def natv():
    from indextts import _native_voice
    _native_voice.lib()
    return _native_voice


@pytest.fixture(scope="module")
def ws(natv):
    return natv.delta_workspace(DEV)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{tname(p[0])}-{tname(p[1])}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_delta_project_against_fp64(natv, ws, shape, pair):
    K, N, c = shape
    tt, tb = pair
    seed = 1000 * SHAPES.index(shape) + 10 * PAIRS.index(pair)
    wb = rnd(K, N, seed=seed, scale=0.02).to(tb)
    wt = (wb.double() + rnd(K, N, seed=seed + 1, scale=0.0016)).to(tt)              # 2 sqrt(4) 0.02^2: a rank-4 LoRA of make_factors at s = 2
    wt_d, wb_d = wt.to(DEV), wb.to(DEV)
    D = (wt.double() - wb.double()).to(DEV)
    D_ctl = (wt.double() - wb.to(torch.bfloat16).double()).to(DEV)
    for trans in (False, True):
        L, rows = (K, K) if trans else (N, N)
        x = rnd(rows, c, seed=seed + 2 + trans).float()
        xd = x.double().to(DEV)
        op, op_ctl = (D.t(), D_ctl.t()) if trans else (D, D_ctl)
        ref, bound = op @ xd, (L + 2) * 2.0 ** -24 * (op.abs() @ xd.abs())
        y = natv.delta_project(wt_d, wb_d, x.to(DEV), trans, ws)
        what = f"delta_{'cols' if trans else 'rows'}<{tname(tt)},{tname(tb)},{c // 16}> K={K} N={N}"
        assert y.shape == ref.shape and y.dtype == torch.float32
        ok(what, y, ref, bound)
        if tb == torch.float16:
            bad(what, "Wb rounded to bf16", y, op_ctl @ xd, bound)
        again = natv.delta_project(wt_d, wb_d, x.to(DEV), trans, ws, out=torch.full_like(y, 7.0))
        assert torch.equal(y, again), what                                           # the same bits, whoever arrives last


def test_k_24_is_refused_without_a_launch(natv, ws):
    from indextts._native import NativeError
    w = torch.zeros(24, 16, dtype=torch.float16, device=DEV)
    y = torch.full((24, 16), 7.0, device=DEV)
    with pytest.raises(NativeError, match=r"K and N must be positive multiples of 16 \(got K=24 N=16\)"):
        natv.delta_project(w, w, torch.ones(16, 16, device=DEV), False, ws, out=y)
    with pytest.raises(NativeError, match=r"c must be 16, 32, 48, 64 or 80 \(got 96\)"):
        natv.delta_project(w[:16], w[:16], torch.ones(16, 96, device=DEV), False, ws)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
