"""ittm_search and ittm_overlap_add on the GPU through the C ABI (libindextts_tempo.so) against
tests/tempo_refs.py: every lag audited given the device's own lag before it, the chain equal to the reference's on the rows
without an ambiguous frame, every output within three fp32 roundings of float64 over the device's lags, nothing written past a
row's K lags or n_out outputs, the same bits on a second run, every row bit-equal to itself alone amid 1e30, every negative
control outside.

Shapes (tempo_refs.CASES): rows of 1, 383, 384, 385, 769, 2400 and 24 000 samples -- a lone sample (all padding), one hop less a
sample, one hop, one more, one window plus a sample, a handful of frames, 33 to 126 frames with two gaps -- at S of 512, 819,
1024, 1280 and 2048, both ends of the range at short and at long rows.  One launch of each kernel, made once and kept."""
import functools

import numpy as np
import pytest
import torch

import tempo_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 1e30
LAG_SENTINEL, Y_SENTINEL = -77777, 777.0


def natm():
    from indextts import _native_tempo
    return _native_tempo


def run(xs, speeds, only=None):
    """The rows in one packed buffer, each at a multiple of 4 elements: ([lags], [outputs]) as numpy, one launch of each kernel.
    only=r: the same buffer with everything but row r's samples at 1e30 -- the other rows and the padding -- and a table of
    that row alone, at the same places in x, offsets and y."""
    N = natm()
    parts, table, x_off, o_off, y_off = [], [], 0, 0, 0
    for x, S in zip(xs, speeds):
        n = x.size
        table.append((x_off, n, o_off, y_off, S, 0))
        parts += [x, np.zeros(-n % 4, dtype=np.float32)]
        x_off += n + (-n % 4)
        o_off += (R.frames(n, S) + 3) & ~3
        y_off += (R.out_len(n, S) + 3) & ~3
    host = np.concatenate(parts + [np.zeros(4, dtype=np.float32)])
    if only is not None:
        keep = host[table[only][0]: table[only][0] + table[only][1]].copy()
        host[:] = HUGE
        host[table[only][0]: table[only][0] + table[only][1]] = keep
    rows = table if only is None else [table[only]]
    xd = torch.from_numpy(host).to(DEV)
    offsets = torch.full((o_off + 4,), LAG_SENTINEL, dtype=torch.int32, device=DEV)
    y = torch.full((y_off + 4,), Y_SENTINEL, dtype=torch.float32, device=DEV)
    window = torch.from_numpy(R.window32()).to(DEV)
    arr, raw = N.table(rows)
    dev = N.upload(raw, DEV)
    N.search(xd, offsets, arr, dev.data_ptr())
    N.overlap_add(xd, offsets, y, window, arr, dev.data_ptr())
    lags, outs = offsets.cpu().numpy(), y.cpu().numpy()
    written_l, written_y = np.zeros(lags.size, bool), np.zeros(outs.size, bool)
    for _, n, o, yo, S, _ in rows:
        written_l[o: o + R.frames(n, S)] = True
        written_y[yo: yo + R.out_len(n, S)] = True
    assert (lags[~written_l] == LAG_SENTINEL).all(), "a lag written past a row's K"
    assert (outs[~written_y] == Y_SENTINEL).all(), "an output written past a row's n_out"
    return ([lags[o: o + R.frames(n, S)].copy() for _, n, o, _, S, _ in rows],
            [outs[yo: yo + R.out_len(n, S)].copy() for _, n, _, yo, S, _ in rows])


@functools.lru_cache(maxsize=None)
def rows():
    return tuple(R.case_rows())


SPEEDS = tuple(S for _, S, _ in R.CASES)


@functools.lru_cache(maxsize=None)
def batch():
    return run(rows(), SPEEDS)


@functools.lru_cache(maxsize=None)
def chains():
    return tuple(R.chain(x, S) for x, S in zip(rows(), SPEEDS))


def test_every_lag_passes_the_decision_audit():
    lags, _ = batch()
    frames = 0
    for x, S, got in zip(rows(), SPEEDS, lags):
        assert got.dtype == np.int32 and got.size == R.frames(x.size, S) and got[0] == 0
        bad = R.audit(x, S, got)
        print(f"tempo search | n {x.size} S {S}: {got.size} lags, {len(bad)} refused by the audit")
        assert bad == [], (x.size, S, bad[:3])
        frames += got.size - 1
    assert frames > 300


def test_the_chain_is_the_reference_where_no_frame_is_ambiguous():
    lags, _ = batch()
    whole = 0
    for x, S, got, ch in zip(rows(), SPEEDS, lags, chains()):
        if any(f.ambiguous for f in ch):
            continue
        assert got[1:].tolist() == [f.d for f in ch], (x.size, S)
        whole += x.size == 24000
    assert whole >= 1
    for x, S, got, ch in zip(rows(), SPEEDS, lags, chains()):            # a silent frame is at lag 0 whatever the row
        assert all(got[f.k] == 0 for f in ch if f.silent)


def test_every_output_is_within_three_roundings_of_float64():
    lags, outs = batch()
    worst = 0.0
    for x, S, off, got in zip(rows(), SPEEDS, lags, outs):
        want, bound = R.overlap_add(x, S, off)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert R.within(got, want, bound), (x.size, S)
        nz = bound > 0
        if nz.any():
            worst = max(worst, float(np.max(np.abs(got[nz] - want[nz]) / bound[nz])))
        assert (got[~nz] == 0).all()
    print(f"tempo overlap_add | worst error / bound {worst:.3f}")
    assert worst > 0.0                                                   # (fp32 did round somewhere: the bound is not met by construction)


def test_a_second_run_gives_the_same_bits():
    lags, outs = batch()
    lags2, outs2 = run(rows(), SPEEDS)
    for a, b, c, d in zip(lags, lags2, outs, outs2):
        assert np.array_equal(a, b) and np.array_equal(c.view(np.uint32), d.view(np.uint32))


def test_every_row_alone_amid_1e30_is_the_row_in_the_batch():
    lags, outs = batch()
    for r in range(len(SPEEDS)):
        (l1,), (y1,) = run(rows(), SPEEDS, only=r)
        assert np.array_equal(l1, lags[r]), R.CASES[r]
        assert np.array_equal(y1.view(np.uint32), outs[r].view(np.uint32)), R.CASES[r]
        assert np.isfinite(y1).all() and np.abs(y1).max() < 40000.0


def test_every_negative_control_falls_outside():
    lags, outs = batch()
    i = [c[:2] for c in R.CASES].index((24000, 1280))
    x, S, off, got, ch = rows()[i], 1280, lags[i], outs[i], chains()[i]
    # one lag moved by one at a frame whose margin exceeds 4 b (judged, like the audit, from the device's own lag before it)
    p, hit = -R.HOP, None
    for k in range(1, off.size):
        c, b = R.scores(np.asarray(x, dtype=np.float64), S, k, p)
        d = int(off[k])
        if hit is None and -R.TOL < d < R.TOL - 1 and b[d + R.TOL] > 0 and min(c[d + R.TOL] - c[d + R.TOL - 1], c[d + R.TOL] - c[d + R.TOL + 1]) > 4 * b.max():
            hit = k
        p = R.nominal(k, S) + d
    assert hit is not None
    for step in (-1, 1):
        moved = off.copy()
        moved[hit] += step
        assert hit in [k for k, _ in R.audit(x, S, moved)]
    assert R.audit(x, S, off, template_at=0)                             # the template from p_(k-1) instead of p_(k-1) + HOP
    s = next(f for f in ch if f.silent)
    flipped = off.copy()
    flipped[s.k] = R.choose(np.zeros(2 * R.TOL), reverse_ties=True)      # the tie rule reversed on a silent frame
    assert flipped[s.k] != 0 and s.k in [k for k, _ in R.audit(x, S, flipped)]
    want, bound = R.overlap_add(x, S, off)
    assert R.within(got, want, bound)
    assert not R.within(got, R.overlap_add(x, S, off, swap_halves=True)[0], bound)       # the window halves swapped
    assert not R.within(got, R.overlap_add(x, S, off, p_shift=1)[0], bound)              # p_k off by one
    assert not R.within(got, R.overlap_add(x, S, off, p_shift=-1)[0], bound)


def test_refusals_launch_nothing():
    from indextts._native import NativeError
    N = natm()
    x = torch.zeros(1000, dtype=torch.float32, device=DEV)
    offsets = torch.full((8,), LAG_SENTINEL, dtype=torch.int32, device=DEV)
    y = torch.full((2000,), Y_SENTINEL, dtype=torch.float32, device=DEV)
    window = torch.from_numpy(R.window32()).to(DEV)
    for row, what in (((0, 1000, 0, 0, 511, 0), "S = 511"), ((0, 1001, 0, 0, 512, 0), "lies outside x"), ((0, 1000, 4, 0, 512, 0), "offsets too small")):
        arr, raw = N.table([row])
        dev = N.upload(raw, DEV)
        with pytest.raises(NativeError, match=rf"ittm_search failed \(code 1\).*{what}"):
            N.search(x, offsets, arr, dev.data_ptr())
    arr, raw = N.table([(0, 1000, 0, 4, 512, 0)])
    dev = N.upload(raw, DEV)
    with pytest.raises(NativeError, match=r"ittm_overlap_add failed \(code 1\).*y too small"):
        N.overlap_add(x, offsets, y, window, arr, dev.data_ptr())
    with pytest.raises(NativeError, match=r"y overlaps x"):
        N.overlap_add(x, offsets, x[4:], window, arr, dev.data_ptr())
    assert bool((offsets == LAG_SENTINEL).all()) and bool((y == Y_SENTINEL).all())
