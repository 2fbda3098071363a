"""Pitch without a GPU (libindextts_pitch.so, indextts/utils/tempo.py): the ninth library's ABI and refusals
through ctypes; pitch_plan's integers against exact rational arithmetic; resample_ratio_ref, the float64 statement of the kernel,
on tones -- the identity at step 1, the peak and the level of a shifted tone, the attenuation above the new Nyquist frequency
against the stop-band figure computed here from the table; and the public surface: pitch=None and 0 run nothing of the feature,
the four whole-utterance calls take the keyword, the streams refuse it, the command lines parse it."""
import ctypes
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_post_wave_cpu import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ittr_abi_version", "ittr_last_error", "ittr_resample_ratio"]
RATE = 24000
ONE = 1 << 32


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_pitch_library_header_and_table_agree():
    from indextts import _native_pitch as natr
    hdr = open(os.path.join(ROOT, "include", "indextts_pitch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ittr_[a-z0-9_]+)\s*\(", code))) == sorted(natr.EXPORTED_SYMBOLS) == NAMES
    assert sorted(s for s in dynamic_symbols(natr.LIB_PATH) if s.startswith("itt")) == NAMES
    lib = ctypes.CDLL(natr.LIB_PATH)
    lib.ittr_abi_version.restype = ctypes.c_int
    assert lib.ittr_abi_version() == natr.ABI_VERSION == 1 == int(re.search(r"#define ITTR_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("HW", 6), ("PHASES", 256), ("TABLE", 2 * 6 * 256 + 4), ("CUTOFF_ONE", 65536), ("CUTOFF_MIN", 32768), ("TILE", natr.TILE)):
        assert int(re.search(rf"#define ITTR_{name} (\d+)", hdr).group(1)) == value == getattr(natr, name)
    for name, value in (("STEP_MIN", 1 << 31), ("STEP_MAX", 1 << 33)):
        assert int(re.search(rf"#define ITTR_{name} (0x[0-9a-f]+)ull", hdr).group(1), 16) == value == getattr(natr, name)
    assert ctypes.sizeof(natr.Row) == 48 and ctypes.sizeof(natr.ResampleRatioArgs) == 64


def test_the_pitch_library_keeps_its_symbols_apart_and_is_built_and_loaded():
    from indextts import _native_pitch as natr, _native_tempo as natm
    assert not any(s.startswith("ittr_") for s in natm.EXPORTED_SYMBOLS + tuple(dynamic_symbols(natm.LIB_PATH)))
    assert not any(s.startswith("ittm_") for s in dynamic_symbols(natr.LIB_PATH))
    assert natr.LIB_PATH.endswith("libindextts_pitch.so") and natr.LIB_PATH != natm.LIB_PATH
    mk = open(os.path.join(ROOT, "index-tts-lora_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(RLIB\)", mk, re.M) and re.search(r"^check:.*\$\(RLIB\)", mk, re.M) and "pitch.hip" in mk
    assert re.search(r"^\trm -rf .*\$\(RLIB\)", mk, re.M)
    assert "_native_pitch.lib()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch
ROW = (0, 1000, 0, 500, 1 << 33, 32768, 0)


def ratio_args(natr, rows, x=FAKE, y=FAKE + 0x200000, table=FAKE + 0x300000, x_elems=1000, y_elems=2000, n_rows=None):
    arr = (natr.Row * len(rows))(*[natr.Row(*r) for r in rows])
    a = natr.ResampleRatioArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.table = x, x_elems, y, y_elems, table
    a.n_rows, a.rows, a.rows_dev = len(rows) if n_rows is None else n_rows, arr, FAKE
    return a, arr


def test_resample_ratio_refusals_launch_nothing():
    from indextts import _native_pitch as natr
    lib = natr.lib()
    cases = [
        (dict(rows=[(0, 0, 0, 500, 1 << 32, 65536, 0)]), b"n = 0 samples"),
        (dict(rows=[(0, 1000, 0, 0, 1 << 32, 65536, 0)]), b"n_out = 0 outputs"),
        (dict(rows=[(0, 1 << 30, 0, 500, 1 << 32, 65536, 0)]), b"1 <= n, n_out < 2^30"),
        (dict(rows=[(0, 1000, 0, 500, (1 << 31) - 1, 65536, 0)]), b"has the step 2147483647"),
        (dict(rows=[(0, 1000, 0, 500, (1 << 33) + 1, 32768, 0)]), b"has the step 8589934593"),
        (dict(rows=[(0, 1000, 0, 500, 1 << 33, 32767, 0)]), b"has the cutoff 32767"),
        (dict(rows=[(0, 1000, 0, 500, 1 << 32, 65537, 0)]), b"has the cutoff 65537"),
        (dict(rows=[(2, 900, 0, 500, 1 << 32, 65536, 0)]), b"no multiple of 4"),
        (dict(rows=[(0, 900, 6, 500, 1 << 32, 65536, 0)]), b"no multiple of 4"),
        (dict(rows=[(4, 1000, 0, 500, 1 << 32, 65536, 0)]), b"lies outside x"),
        (dict(rows=[(-4, 1000, 0, 500, 1 << 32, 65536, 0)]), b"lies outside x"),
        (dict(rows=[ROW, (0, 1000, 1504, 500, 1 << 33, 32768, 0)]), b"row 1 has n_out = 500 outputs: y too small"),
        (dict(rows=[ROW], n_rows=0), b"n_rows must be 1..65535"),
        (dict(rows=[ROW], x=FAKE + 4), b"16-byte aligned"),
        (dict(rows=[ROW], table=FAKE + 8), b"16-byte aligned"),
        (dict(rows=[ROW], y=FAKE + 2), b"y 4-byte aligned"),
        (dict(rows=[ROW], y=FAKE + 400), b"y overlaps x"),
        (dict(rows=[ROW], x=0), b"null pointer"),
        (dict(rows=[ROW], x_elems=-1), b"negative element count"),
    ]
    for kw, what in cases:
        a = ratio_args(natr, **kw)
        assert lib.ittr_resample_ratio(ctypes.byref(a[0]), None) == 1 and what in lib.ittr_last_error(), (what, lib.ittr_last_error())
    assert lib.ittr_resample_ratio(None, None) == 1 and b"null argument struct" in lib.ittr_last_error()


# ------------------------------------------------------------------------------------------------------------- pitch_plan
@pytest.mark.parametrize("speed", [None, 0.8, 1.0, 1.25])
def test_zero_semitones_is_step_one_at_the_speed(speed):
    from indextts.utils import tempo
    rate, step, out_len = tempo.pitch_plan(0, speed)
    assert step == ONE == tempo.STEP_ONE and rate == (1.0 if speed is None else speed)
    assert [out_len(n) for n in (0, 1, 2, 24000)] == [0, 1, 2, 24000]
    assert tempo.TempoEngine.plan(0, speed) == (None if speed is None else tempo.fixed_speed(speed), None)     # ... and the speed= path
    assert tempo.TempoEngine.plan(None, speed) == tempo.TempoEngine.plan(0.0, speed)


def test_an_octave_is_exactly_two_and_a_half():
    from indextts.utils import tempo
    up, down = tempo.pitch_plan(12), tempo.pitch_plan(-12)
    assert (up[0], up[1]) == (0.5, 2 * ONE) and (down[0], down[1]) == (2.0, ONE // 2)
    assert tempo.cutoff_of(2 * ONE) == 32768 and tempo.cutoff_of(ONE // 2) == tempo.cutoff_of(ONE) == 65536
    assert tempo.TempoEngine.plan(12, None) == (512, 2 * ONE) and tempo.TempoEngine.plan(-12, 1.0) == (2048, ONE // 2)
    assert tempo.pitch_plan(12, 2.0)[0] == 1.0 and tempo.pitch_plan(-12, 0.5)[0] == 1.0


@pytest.mark.parametrize("st", [-12, -7, -5, -0.5, 0, 1, 3, 4, 11.9, 12])
def test_out_len_is_the_exact_ceiling_and_monotone(st):
    from indextts.utils import tempo
    rate, step, out_len = tempo.pitch_plan(st)
    p = Fraction(step, ONE)
    assert abs(float(p) - 2.0 ** (st / 12.0)) <= 2.0 ** -32 and abs(rate * float(p) - 1.0) < 1e-9
    for n in (0, 1, 2, 63, 64, 65, 24000):
        assert out_len(n) == math.ceil(Fraction(n) / p), (st, n)
        if n:                                                           # the last output reads inside the row, one more would not
            assert (out_len(n) - 1) * step < n * ONE <= out_len(n) * step
    lens = [out_len(n) for n in range(0, 400)]
    assert all(a <= b for a, b in zip(lens, lens[1:])) and lens[-1] > lens[0]


def test_pitch_plan_refusals_name_both_numbers():
    from indextts.utils import tempo
    for st in (12.01, -12.5, 13, float("nan"), float("inf"), True, "high", [3]):
        with pytest.raises(ValueError, match=r"pitch = .*speed = "):
            tempo.pitch_plan(st, 1.0)
    for st, speed in ((12, 0.5), (-12, 2.0), (4, 0.6), (-4, 1.7), (1, 0.5), (-1, 2.0)):
        with pytest.raises(ValueError, match=rf"pitch = {st} semitones at speed = {speed}.*outside \[0.5, 2.0\]"):
            tempo.pitch_plan(st, speed)
    for speed in (0.4, 2.5, True, "fast"):
        with pytest.raises(ValueError, match="speed = "):
            tempo.pitch_plan(3, speed)
    eng = object.__new__(tempo.TempoEngine)                             # no device: every refusal comes before it is touched
    for kw, what in ((dict(pitch=[1, 2]), "2 pitches for 3 rows"), (dict(pitch=3, speed=[1.0]), "1 speeds for 3 rows"),
                     (dict(pitch=12, speed=0.5), "outside"), (dict(pitch=[0, None, 12.5]), "pitch = 12.5")):
        with pytest.raises(ValueError, match=what):
            eng.shift([torch.zeros(4)] * 3, **kw)


# ----------------------------------------------------------------------------------------------------- the float64 statement
def test_the_table_is_one_filter_family_with_exact_integers():
    from indextts import _native_pitch as natr
    from indextts.utils import tempo
    G = tempo.ratio_table()
    assert G.dtype == torch.float32 and G.shape == (natr.TABLE,)
    g = G.numpy().astype(np.float64)
    whole = g[:: natr.PHASES]
    assert whole[natr.HW] == 1.0 and np.count_nonzero(whole) == 1 and (g[2 * natr.HW * natr.PHASES:] == 0).all()
    k = np.arange(2 * natr.HW * natr.PHASES)
    u = k / natr.PHASES - natr.HW
    want = np.sinc(u) * np.cos(np.pi * u / (2 * natr.HW)) ** 2           # sinc_interp_hann, lowpass_filter_width 6, as resample()
    assert np.max(np.abs(g[: k.size] - want)) <= 2.0 ** -24
    assert np.array_equal(g[: k.size][1:], g[: k.size][1:][::-1])        # symmetric: h(u) = h(-u)


def test_step_one_is_the_identity_bit_for_bit():
    from indextts.utils import tempo
    x = np.random.default_rng(1).uniform(-1, 1, 777).astype(np.float32)
    y = tempo.resample_ratio_ref(x, ONE)
    assert y.shape == (777,) and np.array_equal(y.astype(np.float32).view(np.uint32), x.view(np.uint32)) and np.array_equal(y, x.astype(np.float64))


def peak_hz(v):
    """The spectral peak of v (Hann window, parabolic interpolation of the log magnitude) in Hz at 24 kHz."""
    spec = np.abs(np.fft.rfft(v * np.hanning(v.size)))
    b = int(np.argmax(spec))
    la, lb, lc = np.log(spec[b - 1: b + 2])
    return (b + 0.5 * (la - lc) / (la - 2 * lb + lc)) * RATE / v.size


def rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


def test_a_tone_moves_by_the_ratio_and_keeps_its_level():
    from indextts.utils import tempo
    n = 8192
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / RATE).astype(np.float32)
    _, step, out_len = tempo.pitch_plan(4)
    y = tempo.resample_ratio_ref(x, step)
    assert y.size == out_len(n) >= 4096 + 200
    mid = y[100: 100 + 4096]
    hz, want = peak_hz(mid), 1000.0 * 2.0 ** (4 / 12)
    print(f"pitch ref | +4 semitones: peak {hz:.2f} Hz (want {want:.2f}), rms out / in {rms(mid) / rms(x):.5f}")
    assert abs(hz - want) <= 0.005 * want
    assert abs(rms(mid) / rms(x.astype(np.float64)) - 1.0) <= 0.01


def test_a_tone_above_the_new_nyquist_meets_the_stop_band_figure():
    """p = 2: every output reads an integer position, so the row is filtered by ONE set of taps, w[d] = c h(c d), c = 1/2, taken
    here from the table in float64.  Its stop band starts where the window's main lobe has ended, c / 2 + c / HW cycles a sample
    (8 kHz); the figure is the largest |W| from there to the input's Nyquist frequency, and a tone at 11 kHz -- which folds to
    1 kHz at the new rate -- must come out that much weaker at the least."""
    from indextts import _native_pitch as natr
    from indextts.utils import tempo
    g = tempo.ratio_table().numpy().astype(np.float64)
    c, HW, PH = 0.5, natr.HW, natr.PHASES
    d = np.arange(-2 * HW + 1, 2 * HW)
    w = c * g[((c * d + HW) * PH).astype(int)]                           # (c d + HW) PH is an integer: no blend
    freqs = np.linspace(c / 2 + c / HW, 0.5, 2001)
    W = np.abs(np.exp(-2j * np.pi * freqs[:, None] * d[None, :]) @ w)
    figure = float(W.max())
    assert abs(w.sum() - 1.0) < 1e-3 and figure < 0.02                   # (a low-pass of gain one; the family's side lobes lie below -34 dB)
    n = 8192
    x = np.sin(2 * np.pi * 11000.0 * np.arange(n) / RATE).astype(np.float32)
    y = tempo.resample_ratio_ref(x, 2 * ONE)
    assert y.size == n // 2
    got = rms(y[100:-100]) / rms(x.astype(np.float64))
    print(f"pitch ref | p = 2, 11 kHz: stop-band figure {figure:.3e} ({20 * np.log10(figure):.1f} dB), rms out / in {got:.3e} ({20 * np.log10(got):.1f} dB)")
    assert got <= figure
    low = np.sin(2 * np.pi * 1000.0 * np.arange(n) / RATE).astype(np.float32)        # ... and the pass band passes
    assert abs(rms(tempo.resample_ratio_ref(low, 2 * ONE)[100:-100]) / rms(low.astype(np.float64)) - 1.0) <= 0.01


def test_past_a_rows_ends_the_input_is_zero():
    from indextts.utils import tempo
    for step in (ONE // 2, int(round(2 ** (3 / 12) * ONE)), 2 * ONE):
        x = np.random.default_rng(2).uniform(-1, 1, 65).astype(np.float32)
        padded = np.concatenate([np.zeros(40, np.float32), x, np.zeros(40, np.float32)])
        n_out = -((-65 * ONE) // step)
        a, mass = tempo.resample_ratio_ref(x, step, detail=True)
        assert a.shape == mass.shape == (n_out,) and (mass >= np.abs(a)).all()
        if step == 2 * ONE:                                              # the same positions inside a longer row of zeros: the same sums
            b = tempo.resample_ratio_ref(padded, step)[20: 20 + n_out]
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------- public surface
def test_pitch_none_and_zero_do_not_call_into_the_libraries(monkeypatch):
    from indextts import _native_pitch as natr, _native_tempo as natm
    from indextts.utils import tempo
    calls = {"search": 0, "overlap_add": 0, "resample_ratio": 0}

    def counting(name):
        def stub(*a, **kw):
            calls[name] += 1
        return stub

    monkeypatch.setattr(natm, "search", counting("search"))
    monkeypatch.setattr(natm, "overlap_add", counting("overlap_add"))
    monkeypatch.setattr(natr, "resample_ratio", counting("resample_ratio"))
    eng = tempo.TempoEngine("cpu")                                       # host stand-ins for the rows: nothing here reaches a kernel
    waves = [torch.arange(900, dtype=torch.float32), torch.ones(500), torch.zeros(0)]
    for kw in ({}, dict(pitch=None), dict(pitch=0), dict(pitch=0.0, speed=1.0), dict(pitch=[None, 0, 0.0], speed=[None, 1.0, 1])):
        got = eng.shift(waves, **kw)
        assert all(g is w for g, w in zip(got, waves))
    assert calls == {"search": 0, "overlap_add": 0, "resample_ratio": 0} and eng.launches == 0 and eng._taps is None
    got = eng.shift(waves, pitch=0, speed=1.25)                          # a speed alone: today's two launches, no third
    assert calls == {"search": 1, "overlap_add": 1, "resample_ratio": 0} and eng.launches == 2 and got[2] is waves[2]
    assert [int(g.numel()) for g in got[:2]] == [tempo.out_len(900, 1280), tempo.out_len(500, 1280)]
    got = eng.shift(waves, pitch=[3, None, -5], speed=[None, None, 1.0])
    assert calls == {"search": 2, "overlap_add": 2, "resample_ratio": 1} and eng.launches == 5 and got[1] is waves[1] and got[2] is waves[2]
    rate, step, out_len = tempo.pitch_plan(3)
    assert int(got[0].numel()) == out_len(tempo.out_len(900, tempo.fixed_speed(rate)))
    assert abs(int(got[0].numel()) - 900) <= 2                          # the duration is kept
    got = eng.shift(waves[:1], lengths=[400], pitch=12, speed=2.0)       # speed / p = 1: no time stretch, the resampler alone
    assert calls == {"search": 2, "overlap_add": 2, "resample_ratio": 2} and int(got[0].numel()) == 200


def test_infer_batch_without_a_pitch_runs_nothing_of_the_feature(monkeypatch):
    from indextts import infer as inf

    class Boom:
        plan = staticmethod(inf.TempoEngine.plan)

        def __init__(self, *a, **kw):
            raise AssertionError("TempoEngine was constructed")

    monkeypatch.setattr(inf, "TempoEngine", Boom)
    tts = inf.IndexTTS.__new__(inf.IndexTTS)
    tts.device = torch.device("cpu")
    waves = [torch.arange(5, dtype=torch.float32), torch.zeros(3)]
    tts._batch_tokens = lambda *a, **kw: {"rows": ["codes"]}
    tts._batch_waveforms = lambda st, ev, reuse_prefix: list(waves)
    texts = [torch.tensor([1, 2]), torch.tensor([3])]
    for kw in ({"pitch": None}, {"pitch": 0}, {"pitch": 0.0, "speed": 1.0}, {"pitch": [None, 0]}, {"pitch": [0, 0], "speed": [None, 1.0]}):
        got = tts.infer_batch(torch.zeros(1, 100, 8), texts, **kw)
        assert len(got) == 2 and all(g is w for g, w in zip(got, waves))
    assert not hasattr(tts, "_tempo")
    for kw in ({"pitch": 3}, {"pitch": [None, -2]}, {"pitch": [0, 1], "speed": 1.25}):
        with pytest.raises(AssertionError, match="TempoEngine was constructed"):
            tts.infer_batch(torch.zeros(1, 100, 8), texts, **kw)


def test_the_whole_utterance_calls_take_pitch_and_the_streams_refuse_it():
    from indextts.infer import IndexTTS
    for name in ("infer", "infer_fast", "infer_batch", "infer_queue"):
        p = inspect.signature(getattr(IndexTTS, name)).parameters
        assert "pitch" in p and p["pitch"].default is None and p["pitch"].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream", "serve_stream_queue"):
        assert "pitch" not in inspect.signature(getattr(IndexTTS, name)).parameters, name
    tts = object.__new__(IndexTTS)
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream"):
        with pytest.raises(TypeError, match="the streams do not take pitch="):     # TypeError: what they raise for speed=
            next(iter(getattr(IndexTTS, name)(tts, None, [], pitch=None)))
    with pytest.raises(TypeError, match="pitch"):
        IndexTTS.serve_stream_queue(tts, lambda: None, pitch=3)


def test_every_bad_pitch_is_a_value_error_before_anything_runs():
    from indextts.infer import IndexTTS
    from indextts.utils import tempo
    tts = object.__new__(IndexTTS)                                     # no model, no device: a call that got any further would fail otherwise
    texts = [torch.tensor([1, 2]), torch.tensor([3])]
    for bad in (True, float("nan"), 12.5, -13, "high", [1.0], [1.0, 1.0, 1.0], [1.0, True], [3, 14]):
        for name in ("infer_batch", "infer_queue"):
            with pytest.raises(ValueError, match=name + ".*pitch"):
                getattr(IndexTTS, name)(tts, None, texts, pitch=bad)
    for name in ("infer_batch", "infer_queue"):
        with pytest.raises(ValueError, match=name + r".*pitch = 12 semitones at speed = 0.5"):
            getattr(IndexTTS, name)(tts, None, texts, pitch=[0, 12], speed=[1.0, 0.5])
        with pytest.raises(ValueError, match=name + ".*speed"):
            getattr(IndexTTS, name)(tts, None, texts, pitch=3, speed=2.5)
    for bad in (True, float("nan"), 12.5, "high", [1.0], [3, -3]):
        for name in ("infer", "infer_fast"):
            with pytest.raises(ValueError, match=name + ".*pitch"):
                getattr(IndexTTS, name)(tts, "prompt.wav", "text", None, pitch=bad)
    with pytest.raises(ValueError, match=r"infer: pitch = 12 semitones at speed = 0.5"):
        IndexTTS.infer(tts, "prompt.wav", "text", None, pitch=12, speed=0.5)
    assert IndexTTS._check_pitch(None, 1.25, "x", 3) is None and IndexTTS._check_pitch(0, None, "x") is None
    assert IndexTTS._check_pitch([None, 0, 0.0], [0.8, None, 1.0], "x", 3) is None
    up3 = tempo.pitch_plan(3)
    assert IndexTTS._check_pitch(3, None, "x") == (tempo.fixed_speed(up3[0]), up3[1])
    assert IndexTTS._check_pitch([3, None, 0], [None, 1.25, None], "x", 3) == [(tempo.fixed_speed(up3[0]), up3[1]), (1280, None), (None, None)]


def test_the_command_lines_take_the_pitch():
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    api_src = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    assert re.search(r'"--pitch", type=float, default=None', cli) and "--pitch does not apply to --stream" in cli
    assert '{"pitch": args.pitch}' in cli and "pitch_plan(args.pitch, args.speed)" in cli
    assert re.search(r"pitch: Optional\[float\] = None", api_src)
    assert "pitch_of(req, streaming=True)" in api_src[api_src.index('@app.post("/tts/stream")'):]
    assert "pitch_of(req)" in api_src[api_src.index('@app.post("/tts")'):api_src.index('@app.post("/tts/stream")')]


def test_the_api_field_parses_and_an_empty_one_is_none():
    import api
    from fastapi import HTTPException
    assert api.TTSRequest(text="t").pitch is None and api.pitch_of(api.TTSRequest(text="t")) is None
    assert api.pitch_of(api.TTSRequest(text="t", pitch="3.5")) == 3.5 and api.pitch_of(api.TTSRequest(text="t", pitch=-12, speed=1.0)) == -12.0
    for kw in (dict(pitch=13), dict(pitch=12, speed=0.5), dict(pitch=3, speed=3.0)):
        with pytest.raises(HTTPException) as e:
            api.pitch_of(api.TTSRequest(text="t", **kw))
        assert e.value.status_code == 400
    with pytest.raises(HTTPException) as e:
        api.pitch_of(api.TTSRequest(text="t", pitch=2), streaming=True)
    assert e.value.status_code == 400 and "/tts/stream" in e.value.detail
    assert api.pitch_of(api.TTSRequest(text="t"), streaming=True) is None
    src = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    assert re.search(r'v == "" and k in \([^)]*"pitch"\)', src)          # read_request: an empty form field is no pitch
