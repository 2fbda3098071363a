"""ittr_resample_ratio on the GPU through the C ABI (libindextts_pitch.so) against
tempo.resample_ratio_ref, the float64 statement over the same table, on the kernel's own operands.

Shapes: rows of 1, 2, 63, 64, 65, 1000 and 4097 samples of uniform noise in [-1, 1] and one row of 333 samples that holds a single
1.0 at its first and at its last index (the edges), in ONE ragged batch -- a lone sample, two, a tile's worth of outputs less one /
exactly / plus one at p = 1/2 ... 2, and a row of several tiles (4097 samples are 8194 outputs, nine workgroups, at p = 1/2) -- once
at each of the ratios 1/2, 2^(-4/12), 1, 2^(3/12) and 2, and once more with the ratios dealt over the rows of one batch.  One launch a
batch, made once and kept.

The bound of an output, in units of u = 2^-24, with c = 65536 / cutoff >= 1 the stride factor (a row has at most N = 2 HW c + 1 taps
of non-zero weight), mass = sum |w_j x_j| gain, and D the largest step |G[k + 1] - G[k]| of the table:
    a weight      fma(t, G[k+1] - G[k], G[k]): the difference rounds (u t D at most), then the fma (u |w|)
    the sum       N fmas in a chain: N u mass
    the gain      one product: u |y|
    together      (N + 2) u mass + |x|_max E_blend  =  (2 HW c + 3) u mass + |x|_max E_blend,   E_blend = (2 HW c + 1) u D gain
to first order in u.  The largest error / bound seen is printed (profiles/pitch.txt records it)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 1e30
ONE = 1 << 32
LENGTHS = (1, 2, 63, 64, 65, 1000, 4097)
EDGES = 333
STEPS = (ONE // 2, int(round(2.0 ** (-4 / 12) * ONE)), ONE, int(round(2.0 ** (3 / 12) * ONE)), 2 * ONE)
GUARD = 64


def natr():
    from indextts import _native_pitch
    return _native_pitch


def tempo():
    from indextts.utils import tempo as t
    return t


@functools.lru_cache(maxsize=None)
def rows():
    rng = np.random.default_rng(28)
    xs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in LENGTHS]
    edges = np.zeros(EDGES, dtype=np.float32)
    edges[0] = edges[-1] = 1.0
    return tuple(xs + [edges])


def n_out_of(n, step):
    return -((-n * ONE) // step)


def run(xs, steps, only=None):
    """The rows in one packed buffer, each at a multiple of 4 elements, one launch: [outputs] as numpy.  y lies between two guard
    bands and is NaN all over before the launch: whatever is not an output of a row must still be NaN after it.  only=r: the same
    buffer with everything but row r's samples at 1e30 -- the other rows and the padding -- and a table of that row alone, at
    the same places in x and y."""
    N, T = natr(), tempo()
    parts, table, x_off, y_off = [], [], 0, GUARD
    for x, step in zip(xs, steps):
        n = x.size
        table.append((x_off, n, y_off, n_out_of(n, step), step, T.cutoff_of(step), 0))
        parts += [x, np.zeros(-n % 4, dtype=np.float32)]
        x_off += n + (-n % 4)
        y_off += (n_out_of(n, step) + 3) & ~3
    host = np.concatenate(parts + [np.zeros(4, dtype=np.float32)])
    if only is not None:
        keep = host[table[only][0]: table[only][0] + table[only][1]].copy()
        host[:] = HUGE
        host[table[only][0]: table[only][0] + table[only][1]] = keep
    use = table if only is None else [table[only]]
    xd = torch.from_numpy(host).to(DEV)
    y = torch.full((y_off + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    taps = T.ratio_table().to(DEV)
    arr, raw = N.table(use)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    N.resample_ratio(xd, y, taps, arr, dev.data_ptr())
    outs = y.cpu().numpy()
    written = np.zeros(outs.size, bool)
    for _, _, yo, n_out, _, _, _ in use:
        written[yo: yo + n_out] = True
    assert np.isnan(outs[~written]).all(), "something was written outside a row's outputs"
    assert not np.isnan(outs[written]).any()
    return [outs[yo: yo + n_out].copy() for _, _, yo, n_out, _, _, _ in use]


def mixed_steps():
    return tuple(STEPS[(3 * i + 1) % len(STEPS)] for i in range(len(rows())))


@functools.lru_cache(maxsize=None)
def batch(which):
    """which: an index into STEPS (every row at that ratio), or "mixed"."""
    steps = mixed_steps() if which == "mixed" else (STEPS[which],) * len(rows())
    return steps, run(rows(), steps)


@functools.lru_cache(maxsize=None)
def reference(i, step):
    return tempo().resample_ratio_ref(rows()[i], step, detail=True)


def bound_of(x, step, mass):
    N, T = natr(), tempo()
    g = T.ratio_table().numpy().astype(np.float64)
    D = float(np.max(np.abs(np.diff(g))))
    cutoff = T.cutoff_of(step)
    c, gain, u = N.CUTOFF_ONE / cutoff, cutoff / N.CUTOFF_ONE, 2.0 ** -24
    e_blend = (2 * N.HW * c + 1) * u * D * gain
    return (2 * N.HW * c + 3) * u * mass + float(np.max(np.abs(x))) * e_blend


WHICH = list(range(len(STEPS))) + ["mixed"]


@pytest.mark.parametrize("which", WHICH)
def test_every_output_is_within_the_bound_of_float64(which):
    steps, outs = batch(which)
    worst = 0.0
    for i, (x, step, got) in enumerate(zip(rows(), steps, outs)):
        want, mass = reference(i, step)
        assert got.dtype == np.float32 and got.shape == want.shape == (n_out_of(x.size, step),)
        bound = bound_of(x, step, mass)
        err = np.abs(got.astype(np.float64) - want)
        ratio = float(np.max(err / bound))
        print(f"pitch resample_ratio | n {x.size} step {step / ONE:.6f}: {got.size} outputs, worst error / bound {ratio:.3f}")
        assert (err <= bound).all(), (x.size, step, ratio)
        worst = max(worst, ratio)
    print(f"pitch resample_ratio | batch {which}: worst error / bound {worst:.3f}")
    if which != STEPS.index(ONE):
        assert worst > 0.0                                               # (fp32 did round somewhere: the bound is not met by construction)


def test_ratio_one_is_the_input_bit_for_bit():
    _, outs = batch(STEPS.index(ONE))
    for x, got in zip(rows(), outs):
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    steps, outs = batch("mixed")
    assert ONE in steps
    for x, step, got in zip(rows(), steps, outs):
        if step == ONE:
            assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_the_edges_row_is_the_filter_itself():
    """A 1.0 at index 0 and one at the last index: the outputs near an end are the taps of that sample alone, whatever lies past the
    row counts as zero, and at p = 1/2 every other output is the sample itself."""
    i = len(rows()) - 1
    _, outs = batch(STEPS.index(ONE // 2))
    got = outs[i]
    assert got.size == 2 * EDGES and got[0] == 1.0 and got[2 * (EDGES - 1)] == 1.0
    assert (got[2: 2 * (EDGES - 1): 2] == 0.0).all() and (got[40: 2 * EDGES - 42] == 0.0).all()
    g = tempo().ratio_table().numpy()
    m = np.arange(1, 2 * natr().HW, 2)                                   # output m reads m / 2: the first sample's weight is h(m / 2)
    k = (m + 2 * natr().HW) * natr().PHASES // 2                         # ... an entry of the table itself (t = 0): no rounding at all
    assert np.array_equal(got[m], g[k]) and np.array_equal(got[2 * (EDGES - 1) - m], g[k]) and (g[k] != 0).all()


@pytest.mark.parametrize("which", WHICH)
def test_every_row_alone_amid_1e30_is_the_row_in_the_batch(which):
    steps, outs = batch(which)
    for r in range(len(steps)):
        (y1,) = run(rows(), steps, only=r)
        assert np.array_equal(y1.view(np.uint32), outs[r].view(np.uint32)), (which, r)
        assert np.isfinite(y1).all() and np.abs(y1).max() < 4.0


@pytest.mark.parametrize("which", WHICH)
def test_a_second_run_gives_the_same_bits(which):
    steps, outs = batch(which)
    for a, b in zip(outs, run(rows(), steps)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_row_reads_the_same_bits_at_any_place_in_a_batch():
    """The rows in reverse order: other offsets in x and y, other workgroups -- the same outputs."""
    steps, outs = batch("mixed")
    back = run(rows()[::-1], steps[::-1])
    for a, b in zip(outs, back[::-1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_every_negative_control_falls_outside():
    """The bound is not so wide that it takes anything: the reference read a sample late, blended from the wrong neighbour, or
    without the gain, is outside it."""
    T = tempo()
    i = LENGTHS.index(1000)
    for which in (3, 1):                                                 # 2^(3/12), the strided table; 2^(-4/12), the plain one
        step = STEPS[which]
        _, outs = batch(which)
        x, got = rows()[i], outs[i].astype(np.float64)
        want, mass = reference(i, step)
        bound = bound_of(x, step, mass)
        assert (np.abs(got - want) <= bound).all()
        late = T.resample_ratio_ref(np.concatenate([[0.0], x]), step, n_out=want.size)
        assert not (np.abs(got - late) <= bound).all()
        g = T.ratio_table().numpy().astype(np.float64)
        shifted = np.concatenate([g[1:], [0.0]])                         # every phase one too far
        assert not (np.abs(got - T.resample_ratio_ref(x, step, table=shifted)) <= bound).all()
    step = STEPS[3]
    _, outs = batch(3)
    want, mass = reference(i, step)
    no_gain = want * natr().CUTOFF_ONE / T.cutoff_of(step)
    assert not (np.abs(outs[i] - no_gain) <= bound_of(rows()[i], step, mass)).all()
