"""ittp_frame_stats and ittp_splice on the GPU through the C ABI (libindextts_post.so) against
tests/post_wave_refs.py: the peak exact, the sum of squares within the derived worst case of a 240-term fp32 sum, every spliced
sample within two fp32 roundings of float64, rows isolated bit for bit, every negative control outside, every refusal by message.

Shapes: frame statistics of rows of 1, 239, 240, 241, 4801 and 24 000 samples in one launch (a lone sample, a frame short of one,
one frame, one sample more, 21 frames -- two workgroups -- with a partial one, 100 frames); splices of up to 4801 samples (five
runs).  Each launch is made once and kept."""
import functools

import numpy as np
import pytest
import torch

import post_wave_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 239, 240, 241, 4801, 24000)


def natp():
    from indextts import _native_post
    return _native_post


def packed(rows):
    """fp32 numpy rows in one device buffer, each at a multiple of 4 elements: (x, [(x_off, n)])."""
    parts, table, off = [], [], 0
    for r in rows:
        table.append((off, r.size))
        parts += [r, np.zeros(-r.size % 4, dtype=np.float32)]
        off += r.size + (-r.size % 4)
    return torch.from_numpy(np.concatenate(parts)).to(DEV), table


def run_stats(rows):
    N = natp()
    x, table = packed(rows)
    frames = [R.frames(n) for _, n in table]
    stats = torch.full((len(rows), max(frames), 2), -1.0, dtype=torch.float32, device=DEV)
    arr, raw = N.table(N.Row, table)
    dev, (at,) = N.upload(raw, device=DEV)
    N.frame_stats(x, stats, arr, dev.data_ptr() + at)
    host = stats.cpu().numpy()
    for r, f in enumerate(frames):
        assert (host[r, f:] == -1.0).all()                      # nothing is written past a row's frames
    return tuple(host[r, :f].copy() for r, f in enumerate(frames))


@functools.lru_cache(maxsize=None)
def stat_rows():
    return tuple(R.gauss(n, seed=i) for i, n in enumerate(NS))


@functools.lru_cache(maxsize=None)
def stat_batch():
    return run_stats(stat_rows())


def excess(got_ss, ss64):
    """The largest error of a frame's sum of squares over its bound."""
    with np.errstate(over="ignore"):                             # (a control's empty frame: anything over its zero bound)
        return float(np.max(np.abs(got_ss.astype(np.float64) - ss64) / R.ss_bound(np.maximum(ss64, 1e-300))))


def test_frame_stats_peak_is_exact_and_the_sum_is_within_the_bound():
    worst = 0.0
    for x, got in zip(stat_rows(), stat_batch()):
        ss, pk = R.frame_stats64(x)
        assert got.shape == (R.frames(x.size), 2) and got.dtype == np.float32
        assert np.array_equal(got[:, 1].astype(np.float64), pk), x.size
        e = excess(got[:, 0], ss)
        worst = max(worst, e)
        assert e <= 1.0, (x.size, e)
    print(f"frame_stats | worst error / bound {worst:.3f}")


def test_frame_stats_controls_land_outside():
    for x, got in zip(stat_rows(), stat_batch()):
        n = x.size
        if n > 1:                                                # frames laid one sample late
            assert excess(got[:, 0], R.frame_stats64(x, shift=1)[0]) > 1.0, n
        if n % 240:                                              # the partial frame taken for a full one
            assert excess(got[:, 0], R.frame_stats64(x, partial_as_full=True)[0]) > 1.0, n
        if n >= 4801:                                            # the peak without abs: some frame's largest magnitude is negative
            assert not np.array_equal(got[:, 1].astype(np.float64), R.frame_stats64(x, use_abs=False)[1]), n


def test_frame_stats_rows_are_isolated():
    for x, together in zip(stat_rows(), stat_batch()):
        assert np.array_equal(run_stats((x,))[0].view(np.uint32), together.view(np.uint32)), x.size
    again = run_stats(stat_rows()[::-1])[::-1]                   # another order: other workgroups, other offsets
    for a, b in zip(again, stat_batch()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------- splice
def run_splice(cases):
    """cases: [(x fp32 numpy, pieces, gain, n_out)] -> the rows' outputs (numpy), one launch; y is prefilled with a sentinel."""
    N = natp()
    x, table = packed([c[0] for c in cases])
    rows, pieces, y_off = [], [], 0
    for (x_off, n), (_, pcs, gain, n_out) in zip(table, cases):
        rows.append((x_off, n, y_off, n_out, len(pieces), len(pcs), gain, 0))
        pieces += list(pcs)
        y_off += (n_out + 3) & ~3
    y = torch.full((y_off + 4,), 777.0, dtype=torch.float32, device=DEV)
    ramp = torch.from_numpy(R.ramp32()).to(DEV)
    r_arr, r_raw = N.table(N.OutRow, rows)
    p_arr, p_raw = N.table(N.Piece, pieces)
    dev, (r_at, p_at) = N.upload(r_raw, p_raw, device=DEV)
    try:
        N.splice(x, y, ramp, r_arr, dev.data_ptr() + r_at, p_arr, dev.data_ptr() + p_at)
    except Exception:
        assert bool((y == 777.0).all())                          # refused: nothing was launched, nothing written
        raise
    host = y.cpu().numpy()
    for r in rows:                                               # the padding between rows and the tail keep the sentinel
        assert (host[r[2] + r[3]: (r[2] + r[3] + 3) & ~3] == 777.0).all()
    assert (host[y_off:] == 777.0).all()
    return tuple(host[r[2]: r[2] + r[3]].copy() for r in rows)


@functools.lru_cache(maxsize=None)
def splice_cases():
    a, b, c, d = R.gauss(4801, seed=10), R.gauss(4801, seed=11), R.gauss(2000, seed=12), R.gauss(2000, seed=13)
    return (
        (a, ((0, 0, 4801, 0, 0),), 1.0, 4801),                                                    # a bit copy
        (b, ((0, 0, 4801, 0, 0),), 0.5, 4801),                                                    # exact
        (c, ((1, 0, 240, 0, 120), (3, 240, 241, 120, 120), (241, 481, 1000, 120, 0)), 1.7, 1481),  # odd offsets and lengths
        (d, ((0, 0, 700, 0, 120), (1300, 700, 700, 120, 0)), 0.37, 1400),                         # one cut, both fades
        (d, ((240, 0, 1204, 120, 120),), 2.0, 1204),                                              # trimmed at both ends
        (a[:3], ((0, 0, 3, 0, 0),), 3.0, 3),                                                      # less than one store
    )


@functools.lru_cache(maxsize=None)
def splice_batch():
    return run_splice(splice_cases())


def test_splice_is_within_two_roundings_of_float64():
    for k, ((x, pcs, gain, n_out), got) in enumerate(zip(splice_cases(), splice_batch())):
        want = R.splice64(x, pcs, gain, n_out)
        assert got.shape == (n_out,) and R.within_2ulp(got, want), k
    copy, half = splice_batch()[0], splice_batch()[1]
    assert np.array_equal(copy.view(np.uint32), splice_cases()[0][0].view(np.uint32))
    assert np.array_equal(half, splice_cases()[1][0] * np.float32(0.5))
    # controls: a fade read in the other direction, a source one sample off, the ramp of another length
    x, pcs, gain, n_out = splice_cases()[3]
    got = splice_batch()[3]
    assert not R.within_2ulp(got, R.splice64(x, ((0, 0, 700, 0, 120), (1299, 700, 700, 120, 0)), gain, n_out))
    flipped = R.splice64(x, pcs, gain, n_out)
    flipped[580:700] = (flipped[580:700] / R.ramp32()[::-1].astype(np.float64)) * R.ramp32().astype(np.float64)
    assert not R.within_2ulp(got, flipped)
    assert not R.within_2ulp(got, R.splice64(x, ((0, 0, 700, 0, 0), (1300, 700, 700, 120, 0)), gain, n_out))


def test_splice_rows_are_isolated():
    for case, together in zip(splice_cases(), splice_batch()):
        assert np.array_equal(run_splice((case,))[0].view(np.uint32), together.view(np.uint32))
    again = run_splice(splice_cases()[::-1])[::-1]
    for a, b in zip(again, splice_batch()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_splice_refusals_launch_nothing():
    from indextts._native import NativeError
    x = R.gauss(1000, seed=20)
    for what, pcs, n_out in (("lies outside its source row", ((0, 0, 300, 0, 120), (701, 300, 300, 120, 0)), 600),
                             ("overlaps the destination", ((0, 0, 300, 0, 120), (500, 299, 301, 120, 0)), 600),
                             ("shorter than its fades", ((0, 0, 300, 0, 120), (500, 300, 239, 120, 120)), 539)):
        with pytest.raises(NativeError, match=rf"code 1\).*{what}"):
            run_splice(((x, pcs, 1.0, n_out),))
    N = natp()
    assert N.lib().ittp_last_error().decode().startswith("ittp_splice: piece 1 of row 0 is shorter than its fades")
