"""libindextts_score.so on the device (include/indextts_score.h): ittl_target_logit + ittl_head_nll in the
fp32, bf16 and fp16 forms against the float64 reference of tests/score_refs.py on the kernel's own operands, within its bounds.

Every case is R = 130 rows in one launch (three row tiles, the last partial) with, planted: targets at column 0, V - 1, 1023 and
1024; ignored rows (-1, V, 2^31 - 1) at rows 5, 70 and 100; the pad columns V .. ldw - 1 of W alternately NaN and 1e30; logits
spread over about +-80; pairs of IDENTICAL columns (first and last, in one tile, in two tiles, in two ranges).  For a pair (a, c), a < c, three rows: one
with y = a, the same x with y = c, and an x along column a, whose top is the pair.  One case is computed once and shared."""
import functools
import math

import pytest
import torch

import score_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 130
NAMED = (0, 15, 16, 63, 64, 129)      # tile borders: all carry real targets
IGNORED_ROWS = (5, 70, 100)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
VS = (1, 3, 63, 65, 1024, 1025, 1030, 8194)
GUARD = 64
SENT_F, SENT_I, SENT_B = -12345.5, -77777, 0xA5


def shapes(dtype):
    d0 = 4 if dtype == torch.float32 else 8
    return [(D, V, 0.0) for D in (d0, 40, 1280) for V in VS] + [(1280, 12001, 0.0), (1280, 8194, 3e4), (1280, 8194, -3e4)]


def run(x, W, b, y, V):
    """One ittl_target_logit + ittl_head_nll with sentinels around every output and the workspace -> dict of the outputs (clones)."""
    from indextts import _native_score as nl
    n = x.shape[0]
    f = torch.full((3 * (n + GUARD) + GUARD,), SENT_F, dtype=torch.float32, device=DEV)
    i = torch.full((2 * (n + GUARD) + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    need = nl.ws_bytes(n, V)
    wsb = torch.full((need + 2 * GUARD,), SENT_B, dtype=torch.uint8, device=DEV)
    fs = [f[GUARD + k * (n + GUARD): GUARD + k * (n + GUARD) + n] for k in range(3)]
    is_ = [i[GUARD + k * (n + GUARD): GUARD + k * (n + GUARD) + n] for k in range(2)]
    ws = wsb[GUARD: GUARD + need] if need else None
    nl.target_logit(x, W, b, y, fs[0], V=V)
    nl.head_nll(x, W, b, y, fs[0], fs[1], fs[2], is_[0], is_[1], ws=ws, V=V)
    torch.cuda.synchronize()
    out = dict(t=fs[0].clone(), nll=fs[1].clone(), lse=fs[2].clone(), best=is_[0].clone(), rank=is_[1].clone())
    for k in range(4):
        assert (f[k * (n + GUARD): k * (n + GUARD) + GUARD] == SENT_F).all(), f"float guard {k} overwritten"
    for k in range(3):
        assert (i[k * (n + GUARD): k * (n + GUARD) + GUARD] == SENT_I).all(), f"int guard {k} overwritten"
    assert (wsb[:GUARD] == SENT_B).all() and (wsb[GUARD + need:] == SENT_B).all(), "workspace guard overwritten"
    return out


def same_bits(a, b, rows=None):
    for k in a:
        u, v = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        if not torch.equal(u.view(torch.int32), v.view(torch.int32)):
            return False
    return True


@functools.lru_cache(maxsize=None)
def case(dtype, D, V, bias):
    from indextts import _native_score as nl
    g = torch.Generator().manual_seed(D * 100003 + V * 7 + int(bias > 0))
    x = torch.randn(R, D, generator=g)
    ldw = nl.pitch(V) + 8
    W = (torch.randn(D, ldw, generator=g) * (20.0 / math.sqrt(D))).to(dtype)
    b = torch.randn(V, generator=g) + bias
    y = torch.randint(0, V, (R,), generator=g)
    pairs, used = [], set()
    for a, c in ((0, V - 1), (1, 2), (3, 70), (5, 1029)):
        if c < V and a < c and not {a, c} & used:
            pairs.append((a, c))
            used |= {a, c}
            W[:, c], b[c] = W[:, a], b[a]
    W[:, V:] = torch.tensor([float("nan"), 1e30]).repeat((ldw - V + 1) // 2)[: ldw - V].to(dtype)
    for r, t in zip((0, 15, 16, 63), (0, V - 1, min(1023, V - 1), min(1024, V - 1))):
        y[r] = t
    for r, t in zip(IGNORED_ROWS, (-1, V, 2 ** 31 - 1)):
        y[r] = t
    for i, (a, c) in enumerate(pairs):
        wa = W[:, a].double()
        x[21 + 3 * i] = x[20 + 3 * i]
        y[20 + 3 * i], y[21 + 3 * i] = a, c
        x[22 + 3 * i] = (wa * (60.0 / (wa @ wa).clamp_min(1e-30))).float()
    x, W, b, y = x.to(DEV).contiguous(), W.to(DEV).contiguous(), b.to(DEV).contiguous(), y.to(torch.int32).to(DEV)
    ref = SR.reference(x, W, b, y, V, dtype)
    dev = run(x, W, b, y, V)
    return dict(x=x, W=W, b=b, y=y, V=V, ref=ref, dev=dev, pairs=pairs, dtype=dtype)


def all_cases():
    return [pytest.param(dt, D, V, bias, id=f"{str(dt)[6:]}-D{D}-V{V}" + (f"-bias{bias:+.0e}" if bias else "")) for dt in DTYPES
            for D, V, bias in shapes(dt)]


@pytest.mark.parametrize("dtype,D,V,bias", all_cases())
def test_outputs_within_the_bounds_of_the_float64_reference(dtype, D, V, bias):
    c = case(dtype, D, V, bias)
    ref, dev = c["ref"], c["dev"]
    excess = ((dev["lse"].double() - ref["lse"]).abs() - 2 * ref["E"] - (V + 2) * 2.0 ** -24).max().item()
    print(f"{dtype} D {D} V {V} bias {bias}: max |lse - lse64| {(dev['lse'].double() - ref['lse']).abs().max().item():.3e}, "
          f"max |nll - nll64| {(dev['nll'].double() - ref['nll']).abs().max().item():.3e}, max E {ref['E'].max().item():.3e}, "
          f"excess over the derived terms {excess:.3e}, rows undecided {(~ref['decided']).sum().item()}")
    bad = SR.mismatches(dev, ref, V)
    assert not bad, bad
    fb = SR.float_bound(ref, V)
    for r in NAMED:                                     # the rows at the tile borders, by name: all five outputs
        assert ref["real"][r], r
        assert abs(dev["t"][r].item() - ref["t"][r].item()) <= ref["E"][r].item(), r
        assert abs(dev["lse"][r].item() - ref["lse"][r].item()) <= fb[r].item(), r
        assert abs(dev["nll"][r].item() - ref["nll"][r].item()) <= fb[r].item(), r
        assert abs(dev["rank"][r].item() - ref["rank"][r].item()) <= ref["near"][r].item(), r
        assert 0 <= dev["best"][r].item() < V and (not ref["decided"][r] or dev["best"][r].item() == ref["best"][r].item()), r
    for r in IGNORED_ROWS:                              # the ignore rule
        assert dev["nll"][r].item() == 0.0 and dev["t"][r].item() == 0.0 and dev["rank"][r].item() == -1
        assert 0 <= dev["best"][r].item() < V and math.isfinite(dev["lse"][r].item())
    # planted ties: t has the bits of the streamed logit, so the copy of the target's column compares EQUAL and the smaller id goes
    # first: exactly one more column is ahead of y = c than of y = a; and the pair on top is resolved to a
    ties_checked = 0
    for i, (a, c2) in enumerate(c["pairs"]):
        ra, rc, rt = 20 + 3 * i, 21 + 3 * i, 22 + 3 * i
        assert dev["t"][ra].view(torch.int32).item() == dev["t"][rc].view(torch.int32).item(), (a, c2)
        assert dev["rank"][rc].item() == dev["rank"][ra].item() + 1, (a, c2, dev["rank"][ra].item(), dev["rank"][rc].item())
        if ref["decided"][rt] and ref["best"][rt].item() == a:
            assert dev["best"][rt].item() == a, (a, c2, dev["best"][rt].item())
            ties_checked += 1
    print(f"  planted pairs {len(c['pairs'])}, of which the pair is the decided top of its row and best was checked: {ties_checked}")
    if D >= 40:                                         # ... which is every pair wherever the planted row can dominate: x along column
        assert ties_checked == len(c["pairs"])          # a gives l(a) = 60 + b, the others 60 cos(a, j) |W_j| / |W_a|, cos ~ D^-1/2


@pytest.mark.parametrize("dtype,D,V,bias", all_cases())
def test_same_bits_again_alone_and_amid_garbage(dtype, D, V, bias):
    c = case(dtype, D, V, bias)
    x, W, b, y, dev = c["x"], c["W"], c["b"], c["y"], c["dev"]
    assert same_bits(run(x, W, b, y, V), dev), "a second run differs"
    for r in range(R):                                  # every row alone (R = 1: one partial tile)
        one = run(x[r: r + 1].contiguous(), W, b, y[r: r + 1].contiguous(), V)
        assert all(torch.equal(one[k].view(torch.int32), dev[k][r: r + 1].view(torch.int32)) for k in one), f"row {r} alone differs"
    xg = torch.empty_like(x)
    xg[0::2], xg[1::2] = float("nan"), 1e30
    keep = torch.tensor(NAMED + IGNORED_ROWS + (20, 21, 22), device=DEV)
    xg[keep] = x[keep]
    assert same_bits(run(xg, W, b, y, V), dev, keep), "a row amid NaN / 1e30 rows differs"


@pytest.mark.parametrize("dtype", DTYPES)
def test_negative_controls_fail_the_comparison(dtype):
    """Host-side perturbations of the REFERENCE: each must make the comparison fail, or the comparison shows nothing."""
    c = case(dtype, 40, 8194, 0.0)
    x, W, b, y, V, dev = c["x"], c["W"], c["b"], c["y"], c["V"], c["dev"]
    assert not SR.mismatches(dev, c["ref"], V)
    for name, kw in (("bias left out", dict(drop_bias=True)), ("pad columns included", dict(pad_columns=True)),
                     ("target off by one", dict(target_shift=1)), ("tie rule reversed", dict(reverse_ties=True)),
                     ("one range dropped from the merge", dict(drop_range=3))):
        bad = SR.mismatches(dev, SR.reference(x, W, b, y, V, dtype, **kw), V)
        print(name, {k: len(v) for k, v in bad.items()})
        assert bad, f"{name}: the comparison still passes"


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_masked_by_a_bias_of_minus_infinity_join_as_nothing(dtype):
    """b[j] = -inf masks a column: it adds nothing to lse, is never best and is never ahead of a target -- also column 0, which a
    chain meets while its running maximum is still -inf, and a whole 64-column tile.  E is taken over the other columns."""
    from indextts import _native_score as nl
    D, V, n = 40, 1100, 70
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, D, generator=g).to(DEV)
    W = (torch.randn(D, nl.pitch(V), generator=g) * 3.0).to(dtype).to(DEV)
    b = torch.randn(V, generator=g)
    masked = torch.tensor([0, 3, 69, 1024, V - 1] + list(range(128, 192)))
    b[masked] = -float("inf")
    b = b.to(DEV)
    keep = torch.ones(V, dtype=torch.bool)
    keep[masked] = False
    open_cols = keep.nonzero().reshape(-1).to(DEV)
    y = open_cols[torch.randint(0, open_cols.numel(), (n,), generator=g).to(DEV)].to(torch.int32)
    dev = run(x, W, b, y, V)
    # the same head with the masked columns REMOVED, in float64: what "joins as nothing" means
    ref = SR.reference(x, W[:, open_cols].contiguous(), b[open_cols], torch.searchsorted(open_cols, y.long()), open_cols.numel(), dtype)
    fb = SR.float_bound(ref, V)
    assert torch.isfinite(dev["lse"]).all()
    assert ((dev["lse"].double() - ref["lse"]).abs() <= fb).all() and ((dev["nll"].double() - ref["nll"]).abs() <= fb).all()
    assert ((dev["rank"].long() - ref["rank"]).abs() <= ref["near"]).all()
    assert keep.to(DEV)[dev["best"].long()].all()
    assert (open_cols[ref["best"]] == dev["best"].long())[ref["decided"]].all()
