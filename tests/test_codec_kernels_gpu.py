"""ittc_conv and ittc_nearest_code on the GPU through the C ABI (libindextts_codec.so) against
tests/codec_refs.py: every output of a convolution within (K + 2) 2^-24 (sum |w x| + |b| + |resid|) of float64 on the same fp32
operands, nothing written past a clip's rows, the same bits on a second run, every clip bit-equal to itself alone amid 1e30,
every negative control outside; every code passes the decision audit, equals the float64 argmax where the margin exceeds 2 b,
and the planted ties go to the smaller code.

Shapes.  Convolutions: the small model's six layer forms (the fixture's weights), each over clips of 1, 2, 3, 4, 5, 37 and 160
input rows in ONE launch -- odd lengths under stride 2, rows at clip edges, more than one 64-row tile; and one full-width form
each at seeded weights (300 -> 512 stride 2, 1536 -> 1024 stride 2, 3072 -> 1024 with ReLU-in, ReLU-out and residual,
1024 -> 512 k1) over clips of 5 and 41 rows.  Between the clips of the packed input lies a row of 1e30 that no clip may read.
Search: 64 codes x 32 and 8192 codes x 512 on 1, 15, 16, 17 and 41 rows."""
import functools
import zlib

import numpy as np
import pytest
import torch

import codec_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 1e30
SENTINEL = 777.0
LENS = (1, 2, 3, 4, 5, 37, 160)


def natc():
    from indextts import _native_codec
    return _native_codec


def layout(lens, stride):
    """Clips one after another with one row between them (and before the first): (segs, x_rows, y_rows)."""
    segs, xo, yo = [], 1, 1
    for n in lens:
        segs.append((xo, n, yo))
        xo, yo = xo + n + 1, yo + R.out_rows(n, stride) + 1
    return segs, xo, yo


def run_conv(clips, w, b, stride, flags, resids=None, only=None):
    """The clips ([n_i][Cin] fp32) in one packed buffer, the rows between them at 1e30: the list of their outputs, one launch.
    only=s: the same buffer with everything but clip s at 1e30 and a table of that clip alone, at the same places."""
    N = natc()
    Cout, Cin, taps = w.shape
    segs, x_rows, y_rows = layout([c.shape[0] for c in clips], stride)
    x = np.full((x_rows, Cin), HUGE, dtype=np.float32)
    resid = np.full((y_rows, Cout), HUGE, dtype=np.float32) if flags & R.RESIDUAL else None
    for s, ((x0, n, y0), c) in enumerate(zip(segs, clips)):
        if only is None or only == s:
            x[x0: x0 + n] = c
            if resid is not None:
                resid[y0: y0 + R.out_rows(n, stride)] = resids[s]
    take = segs if only is None else [segs[only]]
    xd, wd, bd = torch.from_numpy(x).to(DEV), N.pack_weight(torch.from_numpy(w).to(DEV)), torch.from_numpy(b).to(DEV)
    rd = None if resid is None else torch.from_numpy(resid).to(DEV)
    y = torch.full((y_rows, Cout), SENTINEL, dtype=torch.float32, device=DEV)
    arr, raw = N.table(take)
    dev = N.upload(raw, DEV)
    N.conv(xd, wd, bd, y, arr, dev.data_ptr(), taps, stride, flags, rd)
    out = y.cpu().numpy()
    written = np.zeros(y_rows, bool)
    for _, n, y0 in take:
        written[y0: y0 + R.out_rows(n, stride)] = True
    assert (out[~written] == SENTINEL).all(), "a row written outside every clip"
    return [out[y0: y0 + R.out_rows(n, stride)].copy() for _, n, y0 in take], (x, resid, segs)


def seeded(name, shape, scale=1.0):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.uniform(-1.0, 1.0, size=shape) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def forms():
    """name -> (w [Cout][Cin][taps], b, stride, flags, clip lengths)."""
    sd = R.fixture()["sd"]
    out = {}
    for name, key, stride, flags in (("enc0", "encoder.0.0", 2, R.RELU_OUT), ("enc1", "encoder.1.0", 2, R.RELU_OUT),
                                     ("net0", "encoder.2.net.0", 1, R.RELU_OUT), ("net2", "encoder.3.net.2", 1, R.RELU_OUT),
                                     ("net4", "encoder.4.net.4", 1, R.RESIDUAL), ("enc5", "encoder.5", 1, 0)):
        out[name] = (sd[key + ".weight"], sd[key + ".bias"], stride, flags, LENS)
    for name, Cout, Cin, taps, stride, flags in (("full300", 512, 100, 3, 2, R.RELU_OUT), ("full1536", 1024, 512, 3, 2, R.RELU_OUT),
                                                 ("full3072", 1024, 1024, 3, 1, R.RELU_IN | R.RELU_OUT | R.RESIDUAL),
                                                 ("full1024", 512, 1024, 1, 1, 0)):
        out[name] = (seeded(name + "w", (Cout, Cin, taps), (taps * Cin) ** -0.5), seeded(name + "b", (Cout,), 0.1), stride, flags, (5, 41))
    return out


NAMES = ("enc0", "enc1", "net0", "net2", "net4", "enc5", "full300", "full1536", "full3072", "full1024")


@functools.lru_cache(maxsize=None)
def inputs(name):
    w, b, stride, flags, lens = forms()[name]
    clips = [seeded(f"{name}x{i}", (n, w.shape[1]), 2.0) for i, n in enumerate(lens)]
    resids = [seeded(f"{name}r{i}", (R.out_rows(n, stride), w.shape[0]), 2.0) for i, n in enumerate(lens)] if flags & R.RESIDUAL else None
    return clips, resids


@functools.lru_cache(maxsize=None)
def batch(name):
    w, b, stride, flags, _ = forms()[name]
    clips, resids = inputs(name)
    return run_conv(clips, w, b, stride, flags, resids)


@functools.lru_cache(maxsize=None)
def reference(name):
    w, b, stride, flags, _ = forms()[name]
    _, (x, resid, segs) = batch(name)
    return R.conv(x, w, b, segs, stride, flags, resid)


@pytest.mark.parametrize("name", NAMES)
def test_every_output_is_within_the_fp32_bound_of_float64(name):
    outs, _ = batch(name)
    want, bound = reference(name)
    w, _, stride, flags, lens = forms()[name]
    worst = 0.0
    for s, got in enumerate(outs):
        assert got.dtype == np.float32 and got.shape == want[s].shape == (R.out_rows(lens[s], stride), w.shape[0])
        assert np.isfinite(got).all()
        assert R.within(got, want[s], bound[s]), (name, lens[s], float(np.max(np.abs(got - want[s]) / bound[s])))
        worst = max(worst, float(np.max(np.abs(got - want[s]) / bound[s])))
    print(f"codec conv | {name}: K = {w.shape[1] * w.shape[2]}, worst error / bound {worst:.4f}")
    assert worst > 0.0                                                   # (fp32 did round somewhere: the bound is not met by construction)


@pytest.mark.parametrize("name", NAMES)
def test_a_second_run_gives_the_same_bits(name):
    w, b, stride, flags, _ = forms()[name]
    again, _ = run_conv(*inputs(name)[:1], w, b, stride, flags, inputs(name)[1])
    for a, c in zip(batch(name)[0], again):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_every_clip_alone_amid_1e30_is_the_clip_in_the_batch(name):
    w, b, stride, flags, lens = forms()[name]
    clips, resids = inputs(name)
    for s in range(len(lens)):
        (alone,), _ = run_conv(clips, w, b, stride, flags, resids, only=s)
        assert np.array_equal(alone.view(np.uint32), batch(name)[0][s].view(np.uint32)), (name, lens[s])


def outside(name, **variant):
    """Does the device's output of `name` fall outside the bound around the variant, on some clip?"""
    w, b, stride, flags, _ = forms()[name]
    outs, (x, resid, segs) = batch(name)
    _, bound = reference(name)
    with np.errstate(all="ignore"):
        want, _ = R.conv(x, w, b, segs, stride, flags, resid, **variant)
    return any(not R.within(got, want[s], bound[s]) for s, got in enumerate(outs))


def test_every_negative_control_falls_outside():
    for name in ("enc0", "net0", "full300", "full3072"):
        assert outside(name, neighbour=True), name                       # a clip padded with its neighbour's rows, not zeros
        assert outside(name, reverse_taps=True), name
    for name in ("enc0", "enc1", "full300", "full1536"):                 # the stride-2 phase off by one, either way
        assert outside(name, phase=1) and outside(name, phase=-1), name
    for name in ("enc0", "net0", "full1536"):                            # the ReLU on the wrong side
        assert outside(name, swap_relu=True), name
    for name in ("net4", "full3072"):
        assert outside(name, drop_residual=True), name
    for name in NAMES:                                                   # (and the variants' machinery takes the reference itself)
        assert not outside(name)


# ------------------------------------------------------------------------------------------------------------- the search
def run_nearest(z, embed, h=None, with_score=True):
    N = natc()
    zd, ed = torch.from_numpy(z).to(DEV), torch.from_numpy(embed).to(DEV)
    hd = torch.from_numpy(R.half_norms32(embed) if h is None else h).to(DEV)
    n = z.shape[0]
    code = torch.full((n + 4,), -7, dtype=torch.int32, device=DEV)
    score = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    nb = N.ws_bytes(n, embed.shape[1])
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV) if nb else None
    N.nearest_code(zd, ed, hd, code[:n], score[:n] if with_score else None, ws)
    c, s = code.cpu().numpy(), score.cpu().numpy()
    assert (c[n:] == -7).all() and (s[n:] == SENTINEL).all() and (with_score or (s == SENTINEL).all())
    return c[:n].copy(), s[:n].copy()


@functools.lru_cache(maxsize=None)
def book(J, D):
    rng = np.random.default_rng(J + D)
    e = rng.standard_normal((D, J)).astype(np.float32)
    if J == 8192:
        e[:, 8191] = e[:, 0]            # the first code of the first range and the last code of the last
        e[:, 1024] = e[:, 1023]         # the last code of a range and the first of the next
        e[:, 4100] = e[:, 70]           # two ranges apart
        e[:, 77] = e[:, 5]              # one range, two tiles
        e[:, 200] = 3.0 * e[:, 100]     # a long code along a short one: nearer to it only if h is left out
    else:
        e[:, 63] = e[:, 0]
        e[:, 41] = e[:, 9]
        e[:, 30] = 3.0 * e[:, 20]
    return e


TIES = {8192: ((0, 8191), (1023, 1024), (70, 4100), (5, 77)), 64: ((0, 63), (9, 41))}
SHORT = {8192: 100, 64: 20}


@functools.lru_cache(maxsize=None)
def rows_of(J, D, n):
    """n rows: the planted ties first (a row AT a duplicated column: both copies score the same bits), then a row at one of
    the last 64 codes, a row at the short code of SHORT, then rows that lie between codes like an encoder's output does."""
    e = book(J, D)
    rng = np.random.default_rng(1000 * n + J)
    z = (0.6 * e[:, rng.integers(0, J, size=n)].T + 0.5 * rng.standard_normal((n, D))).astype(np.float32)
    for r, (a, _) in enumerate(TIES[J]):
        if r < n:
            z[r] = e[:, a]
    if n > len(TIES[J]):
        z[len(TIES[J])] = e[:, J - 3]
    if n > len(TIES[J]) + 1:
        z[len(TIES[J]) + 1] = e[:, SHORT[J]]
    return z


CASES = [(64, 32, n) for n in (1, 15, 16, 17, 41)] + [(8192, 512, n) for n in (1, 15, 16, 17, 41)]


@functools.lru_cache(maxsize=None)
def searched(J, D, n):
    return run_nearest(rows_of(J, D, n), book(J, D))


@pytest.mark.parametrize("J,D,n", CASES)
def test_every_code_passes_the_decision_audit(J, D, n):
    z, e = rows_of(J, D, n), book(J, D)
    codes, score = searched(J, D, n)
    bad, decided = R.audit(z, e, codes)
    print(f"codec nearest | J {J} D {D} rows {n}: {decided} rows decided by a margin above 2 b, {len(bad)} refused by the audit")
    assert bad == []
    s, b = R.scores(z, e)
    assert np.all(np.abs(score - s[np.arange(n), codes]) <= b[np.arange(n), codes])         # the winning score is the winner's
    for r, (a, c) in enumerate(TIES[J]):                                                   # the planted ties: the smaller code
        if r < n:
            assert s[r, a] == s[r, c] == s[r].max() and codes[r] == a, (r, a, c, codes[r])
    if n > len(TIES[J]):
        assert codes[len(TIES[J])] == J - 3
    if n > len(TIES[J]) + 1:
        assert codes[len(TIES[J]) + 1] == SHORT[J]
    again, score2 = run_nearest(z, e, with_score=False)
    assert np.array_equal(codes, again)


def test_a_row_is_the_same_in_any_batch():
    z, e = rows_of(8192, 512, 41), book(8192, 512)
    codes, score = searched(8192, 512, 41)
    amid = np.full((66, 512), HUGE, dtype=np.float32)
    amid[65] = z[40]
    with np.errstate(all="ignore"):
        c1, s1 = run_nearest(amid, e)
    assert c1[65] == codes[40] and s1[65].view(np.uint32) == score[40].view(np.uint32)
    c2, s2 = run_nearest(z[7:8], e)
    assert c2[0] == codes[7] and s2[0].view(np.uint32) == score[7].view(np.uint32)


def test_the_search_controls_fall_outside():
    for J, D in ((64, 32), (8192, 512)):
        z, e = rows_of(J, D, 41), book(J, D)
        codes, _ = searched(J, D, 41)
        s, _ = R.scores(z, e)
        assert R.audit(z, e, R.choose(s))[0] == []
        assert R.audit(z, e, R.choose(R.scores(z, e, omit_h=True)[0]))[0], "h omitted"
        flipped = R.choose(s, reverse_ties=True)
        tied = np.nonzero(flipped != R.choose(s))[0]                    # the rows whose winner is a duplicated column: exact ties
        assert set(range(len(TIES[J]))) <= set(tied.tolist())
        assert all(flipped[r] == c for r, (_, c) in enumerate(TIES[J]))
        assert np.all(codes[tied] == R.choose(s)[tied]) and np.all(codes[tied] < flipped[tied])     # the tie rule reversed: the larger copy
        assert R.audit(z, e, R.choose(s, skip_last=64 if J == 8192 else 16))[0], "the last tile of codes skipped"


def test_refusals_launch_nothing():
    from indextts._native import NativeError
    N = natc()
    x = torch.zeros(8, 100, dtype=torch.float32, device=DEV)
    w = N.pack_weight(torch.zeros(32, 100, 3, device=DEV))
    b = torch.zeros(32, dtype=torch.float32, device=DEV)
    y = torch.full((8, 32), SENTINEL, dtype=torch.float32, device=DEV)
    for segs, stride, what in ((((0, 9, 0),), 2, "lies outside x"), (((0, 8, 5),), 2, "lies outside y"), (((0, 8, 1),), 1, "lies outside y"),
                               (((0, 0, 0),), 2, "x_len = 0")):
        arr, raw = N.table(segs)
        dev = N.upload(raw, DEV)
        with pytest.raises(NativeError, match=rf"ittc_conv failed \(code 1\).*{what}"):
            N.conv(x, w, b, y, arr, dev.data_ptr(), 3, stride, 0)
    arr, raw = N.table([(0, 8, 0)])
    dev = N.upload(raw, DEV)
    with pytest.raises(NativeError, match="the pack does not match"):
        N.conv(x, w, b, y, arr, dev.data_ptr(), 1, 2, 0)
    with pytest.raises(NativeError, match="taps = 2"):
        N.conv(x, w, b, y, arr, dev.data_ptr(), 2, 2, 0)
    both = torch.zeros(16, 100, dtype=torch.float32, device=DEV)
    with pytest.raises(NativeError, match="y overlaps x"):
        N.conv(both[:8], N.pack_weight(torch.zeros(100, 100, 1, device=DEV)), torch.zeros(100, device=DEV), both[4:12], arr, dev.data_ptr(), 1, 1, 0)
    assert bool((y == SENTINEL).all()) and bool((both == 0).all())
    code = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    e = torch.zeros(32, 2048, dtype=torch.float32, device=DEV)
    with pytest.raises(NativeError, match="ws must be"):
        N.nearest_code(torch.zeros(4, 32, device=DEV), e, torch.zeros(2048, device=DEV), code)
    with pytest.raises(NativeError, match="ws too small"):
        N.nearest_code(torch.zeros(4, 32, device=DEV), e, torch.zeros(2048, device=DEV), code, None, torch.zeros(48, dtype=torch.uint8, device=DEV))
    assert bool((code == -7).all())
