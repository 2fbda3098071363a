"""PostWaveEngine.process on the GPU (indextts/utils/post_wave.py) against the float64 restatement of
tests/post_wave_refs.py: sine bursts at -12 dBFS, separated and framed by digital silence or by noise at -70 dBFS, trim_db = -45.

Every frame lies more than 20 dB from the threshold, and the test asserts, from the restatement alone, that every frame's margin
exceeds the frame-statistics bound: no decision can flip on the device, so the engine's pieces must EQUAL the restatement's, its
samples lie within the splice bound, and the level lands where the settings say.

The RMS bound: the gain comes from the device's sums, each within (240 + 1) 2^-24 of float64, so the energy is within d = 241 u
(u = 2^-24) and the gain within d / 2 + d^2; the gain is rounded down to fp32 (2 u) and each sample carries two roundings (2 u):
the measured RMS of the speech is the target within (d / 2 + 4 u + d^2) relative.  Where the ceiling binds, the result's peak is
the ceiling within 8 u: the ceiling and the gain are each rounded down to fp32 (2 u each), the gain may step down once more
(2 u), and the product is rounded (u)."""
import functools

import numpy as np
import pytest
import torch

import post_wave_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRIM = -45.0
LAYOUTS = {
    "two bursts, digital silence": dict(layout=[("q", 30), ("s", 40), ("q", 25), ("s", 30), ("q", 20)], floor_db=None, tail=0),
    "two bursts, noise floor": dict(layout=[("q", 12), ("s", 50), ("q", 11), ("s", 20), ("q", 40)], floor_db=-70.0, tail=131),
    "speech from the first sample": dict(layout=[("s", 25), ("q", 30), ("s", 3), ("q", 1)], floor_db=-70.0, tail=7),
    "one short burst": dict(layout=[("q", 3), ("s", 1), ("q", 2)], floor_db=None, tail=1),
    "nothing but noise": dict(layout=[("q", 21)], floor_db=-70.0, tail=100),
    "nothing but zeros": dict(layout=[("q", 5)], floor_db=None, tail=17),
}
SETTINGS = {
    "trim, cap, level": dict(trim_db=TRIM, max_pause_ms=100.0, target_rms_db=-20.0),
    "trim and a ceiling that binds": dict(trim_db=TRIM, keep_ms=20.0, target_rms_db=-3.0, peak_db=-6.0),
    "peak alone": dict(peak_db=-3.0),
}


@functools.lru_cache(maxsize=None)
def engine():
    from indextts.utils.post_wave import PostWaveEngine
    return PostWaveEngine(DEV)


@functools.lru_cache(maxsize=None)
def rows():
    return tuple(R.bursts(seed=i, **kw) for i, kw in enumerate(LAYOUTS.values()))


@functools.lru_cache(maxsize=None)
def processed(setting):
    """The six rows through the engine in ONE call under `setting`: (outputs as numpy, plans)."""
    from indextts.utils.post_wave import PostProcess
    eng, plans = engine(), []
    before = eng.launches
    outs = eng.process([torch.from_numpy(x).to(DEV) for x in rows()], PostProcess(**SETTINGS[setting]), plans_out=plans)
    assert eng.launches == before + 2
    return tuple(o.cpu().numpy() for o in outs), tuple(plans)


def test_no_decision_can_flip():
    """From float64 alone: every frame's level is more than 20 dB from the threshold, which is far more than the bound on the
    device's sum of squares moves it (241 x 2^-24 relative: 6e-5 dB)."""
    floor = R.FULL ** 2 * 10.0 ** (TRIM / 10.0)
    for name, x in zip(LAYOUTS, rows()):
        ss, _ = R.frame_stats64(x)
        cnt = np.array([R.FRAME] * (len(ss) - 1) + [x.size - R.FRAME * (len(ss) - 1)], dtype=np.float64)
        for f, (s, c) in enumerate(zip(ss, cnt)):
            assert abs(R.frame_db(s, c) - TRIM) > 20.0, (name, f, R.frame_db(s, c))
            assert abs(s / c - floor) > R.ss_bound(s) / c, (name, f)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_engine_is_the_restatement(setting):
    kw = SETTINGS[setting]
    outs, plans = processed(setting)
    stats = engine().frame_stats([torch.from_numpy(x).to(DEV) for x in rows()])
    u, d = 2.0 ** -24, 241 * 2.0 ** -24
    for name, x, got, plan, st in zip(LAYOUTS, rows(), outs, plans, stats):
        ss, pk = R.frame_stats64(x)
        pieces, gain, n_out = R.plan64(ss, pk, x.size, **kw)
        assert list(plan.pieces) == pieces and plan.n_out == n_out == got.size, (name, plan, pieces)
        assert abs(plan.gain - gain) <= (d / 2 + d * d + 2 * u) * gain, (name, plan.gain, gain)
        # the samples, over the gain the engine used (its statistics are the device's)
        assert R.within_2ulp(got, R.splice64(x, plan.pieces, plan.gain, n_out)), name
        # ... which is the plan of the device's own statistics
        assert plan == type(plan)(*_as_plan(R.plan64(st[:, 0].astype(np.float64), st[:, 1].astype(np.float64), x.size, **kw), plan.gain)), name
        if name == "nothing but zeros" or (name.startswith("nothing but") and "trim_db" in kw):      # no frame above the threshold
            assert np.array_equal(got.view(np.uint32), x.view(np.uint32)) and plan.gain == 1.0      # unchanged
            continue
        ceiling_db = kw.get("peak_db", -1.0 if "target_rms_db" in kw else None)
        if ceiling_db is not None:
            assert float(np.abs(got).max()) <= R.FULL * 10.0 ** (ceiling_db / 20.0), name
        # the speech of the result: the loud frames, found through the pieces (the fades lie in the kept silence)
        if "trim_db" in kw:
            loud = [f for f in range(len(ss)) if R.frame_db(ss[f], R.FRAME if f < len(ss) - 1 else x.size - R.FRAME * f) >= TRIM]
            sq = n = 0.0
            for f in loud:
                src, dst, m, fi, fo = next(p for p in plan.pieces if p[0] <= f * R.FRAME < p[0] + p[2])
                a = dst + f * R.FRAME - src
                assert f * R.FRAME - src >= fi and src + m - (f + 1) * R.FRAME >= fo
                seg = got[a:a + R.FRAME].astype(np.float64)
                sq, n = sq + float(np.sum(seg * seg)), n + seg.size
            rms_db = 10.0 * np.log10(sq / n / R.FULL ** 2)
            binds = gain * float(pk.max()) >= 0.999 * R.FULL * 10.0 ** (ceiling_db / 20.0)
            if not binds:
                assert abs(np.sqrt(sq / n) / (R.FULL * 10.0 ** (kw["target_rms_db"] / 20.0)) - 1.0) <= d / 2 + 4 * u + d * d, (name, rms_db)
            else:
                assert rms_db < kw["target_rms_db"] and setting == "trim and a ceiling that binds"
                assert float(np.abs(got).max()) >= (1 - 8 * u) * R.FULL * 10.0 ** (ceiling_db / 20.0)    # lowered to the ceiling, no further
        else:
            assert float(np.abs(got).max()) >= (1 - 8 * u) * R.FULL * 10.0 ** (ceiling_db / 20.0)        # peak normalisation reaches it


def _as_plan(p64, gain):
    pieces, g, n_out = p64
    assert abs(g - gain) <= 2.0 ** -23 * gain                   # (the two float64 routes may round to neighbouring fp32 values)
    return tuple(pieces), gain, n_out


def test_rows_are_isolated_and_empty_rows_pass():
    from indextts.utils.post_wave import PostProcess
    pp = PostProcess(**SETTINGS["trim, cap, level"])
    outs, _ = processed("trim, cap, level")
    eng = engine()
    for x, together in zip(rows()[:3], outs[:3]):
        alone = eng.process([torch.from_numpy(x).to(DEV)], pp)[0].cpu().numpy()
        assert np.array_equal(alone.view(np.uint32), together.view(np.uint32))
    empty = torch.zeros(0, device=DEV)
    plans = []
    got = eng.process([empty, torch.from_numpy(rows()[0]).to(DEV)[1:], empty], pp, plans_out=plans)      # a view at an odd address
    assert got[0].numel() == 0 and got[2].numel() == 0 and plans[0] is None and plans[2] is None and got[1].numel() == plans[1].n_out
    assert eng.process([], pp) == [] and eng.process([empty], pp)[0].numel() == 0
    with pytest.raises(ValueError, match="fp32 tensor"):
        eng.process([torch.zeros(10)], pp)
    with pytest.raises(TypeError, match="PostProcess"):
        eng.process([empty], dict(trim_db=-45))
