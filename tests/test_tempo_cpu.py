"""The speaking rate without a GPU (libindextts_tempo.so, indextts/utils/tempo.py): the sixth library's ABI
and refusals through ctypes, the length arithmetic against the float64 restatement of tests/tempo_refs.py, the restatement's own
sanity and the condition on the audit's inputs, and the public surface: speed=None and 1.0 run nothing of the feature, the four
whole-utterance calls take the keyword and the streams refuse it."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tempo_refs as R
from test_post_wave_cpu import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ittm_abi_version", "ittm_last_error", "ittm_overlap_add", "ittm_search"]


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_tempo_library_header_and_table_agree():
    from indextts import _native_tempo as natm
    hdr = open(os.path.join(ROOT, "include", "indextts_tempo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ittm_[a-z0-9_]+)\s*\(", code))) == sorted(natm.EXPORTED_SYMBOLS) == NAMES
    assert sorted(s for s in dynamic_symbols(natm.LIB_PATH) if s.startswith("itt")) == NAMES
    lib = ctypes.CDLL(natm.LIB_PATH)
    lib.ittm_abi_version.restype = ctypes.c_int
    assert lib.ittm_abi_version() == natm.ABI_VERSION == 1 == int(re.search(r"#define ITTM_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("HOP", 384), ("WIN", 768), ("TOL", 192), ("SPEED_ONE", 1024), ("SPEED_MIN", 512), ("SPEED_MAX", 2048), ("RUN", natm.RUN)):
        assert int(re.search(rf"#define ITTM_{name} (\d+)", hdr).group(1)) == value == getattr(natm, name)
    assert (R.HOP, R.WIN, R.TOL, R.ONE, R.S_MIN, R.S_MAX) == (384, 768, 192, 1024, 512, 2048)
    assert ctypes.sizeof(natm.Row) == 40 and (ctypes.sizeof(natm.SearchArgs), ctypes.sizeof(natm.OverlapAddArgs)) == (56, 80)


def test_the_six_libraries_keep_their_symbols_apart():
    from indextts import _native, _native_audio as nata, _native_out as nato, _native_post as natp, _native_tempo as natm, _native_voice as natv
    others = (_native, nata, nato, natp, natv)
    for other in others:
        assert not any(s.startswith("ittm_") for s in other.EXPORTED_SYMBOLS)
        assert not any(s.startswith("ittm_") for s in dynamic_symbols(other.LIB_PATH))
    lib = ctypes.CDLL(natm.LIB_PATH)
    for other in others:
        for s in other.EXPORTED_SYMBOLS:
            assert not hasattr(lib, s), s
    paths = [m.LIB_PATH for m in others + (natm,)]
    assert len(set(paths)) == 6 and natm.LIB_PATH.endswith("libindextts_tempo.so")


def test_build_names_the_sixth_library():
    mk = open(os.path.join(ROOT, "index-tts-lora_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(MLIB\)", mk, re.M) and re.search(r"^check:.*\$\(MLIB\)", mk, re.M) and "tempo.hip" in mk
    assert re.search(r"^\trm -rf .*\$\(MLIB\)", mk, re.M)
    assert "_native_tempo.lib()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch


def search_args(natm, rows, x=FAKE, offsets=FAKE + 0x100000, x_elems=1000, offsets_elems=64, n_rows=None):
    arr = (natm.Row * len(rows))(*[natm.Row(*r) for r in rows])
    a = natm.SearchArgs()
    a.x, a.x_elems, a.offsets, a.offsets_elems = x, x_elems, offsets, offsets_elems
    a.n_rows, a.rows, a.rows_dev = len(rows) if n_rows is None else n_rows, arr, FAKE
    return a, arr


def add_args(natm, rows, x=FAKE, offsets=FAKE + 0x100000, y=FAKE + 0x200000, window=FAKE + 0x300000, x_elems=1000, offsets_elems=64,
             y_elems=2000, n_rows=None):
    arr = (natm.Row * len(rows))(*[natm.Row(*r) for r in rows])
    a = natm.OverlapAddArgs()
    a.x, a.x_elems, a.offsets, a.offsets_elems, a.y, a.y_elems, a.window = x, x_elems, offsets, offsets_elems, y, y_elems, window
    a.n_rows, a.rows, a.rows_dev = len(rows) if n_rows is None else n_rows, arr, FAKE
    return a, arr


ROW = (0, 1000, 0, 0, 512, 0)       # 1000 samples at half speed: n_out = 2000, K = 7


def test_search_refusals_through_ctypes():
    from indextts import _native_tempo as natm
    lib = natm.lib()

    def refused(what, rows=(ROW,), **kw):
        a = search_args(natm, rows, **kw)
        assert lib.ittm_search(ctypes.byref(a[0]), None) == 1 and what in lib.ittm_last_error(), lib.ittm_last_error()

    assert lib.ittm_search(None, None) == 1 and b"null argument struct" in lib.ittm_last_error()
    refused(b"null pointer", x=None)
    refused(b"null pointer", offsets=None)
    refused(b"16-byte aligned", x=FAKE + 4)
    refused(b"n_rows must be", n_rows=0)
    refused(b"n = 0 samples", rows=((0, 0, 0, 0, 512, 0),))
    refused(b"lies outside x", x_elems=999)
    refused(b"lies outside x", rows=((4, 1000, 0, 0, 512, 0),))
    refused(b"no multiple of 4", rows=((2, 900, 0, 0, 512, 0),))
    refused(b"no multiple of 4", rows=((0, 1000, 6, 0, 512, 0),))
    refused(b"S = 511", rows=((0, 1000, 0, 0, 511, 0),))
    refused(b"S = 2049", rows=((0, 1000, 0, 0, 2049, 0),))
    refused(b"K = 7 frames: offsets too small", offsets_elems=6)
    refused(b"row 1 has K = 7 frames: offsets too small", rows=(ROW, (0, 1000, 8, 0, 512, 0)), offsets_elems=14)


def test_overlap_add_refusals_through_ctypes():
    from indextts import _native_tempo as natm
    lib = natm.lib()

    def refused(what, rows=(ROW,), **kw):
        a = add_args(natm, rows, **kw)
        assert lib.ittm_overlap_add(ctypes.byref(a[0]), None) == 1 and what in lib.ittm_last_error(), lib.ittm_last_error()

    assert lib.ittm_overlap_add(None, None) == 1 and b"null argument struct" in lib.ittm_last_error()
    refused(b"null pointer", window=None)
    refused(b"null pointer", y=None)
    refused(b"16-byte aligned", y=FAKE + 0x200000 + 8)
    refused(b"16-byte aligned", window=FAKE + 0x300000 + 4)
    refused(b"n_rows must be", n_rows=0)
    refused(b"n = 0 samples", rows=((0, 0, 0, 0, 512, 0),))
    refused(b"lies outside x", x_elems=999)
    refused(b"no multiple of 4", rows=((0, 1000, 0, 2, 512, 0),))
    refused(b"S = 0", rows=((0, 1000, 0, 0, 0, 0),))
    refused(b"K = 7 frames: offsets too small", offsets_elems=6)
    refused(b"n_out = 2000 outputs: y too small", y_elems=1999)
    refused(b"n_out = 2000 outputs: y too small", rows=((0, 1000, 0, 4, 512, 0),))
    refused(b"y overlaps x", y=FAKE + 4 * 996)                         # y starts inside x's last 16 bytes
    refused(b"y overlaps x", x=FAKE + 0x200000 + 4 * 1996)             # x starts inside y


# ------------------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("S", [512, 819, 1024, 1280, 2048])
@pytest.mark.parametrize("n", [1, 383, 384, 385, 768, 769])
def test_lengths_are_the_restatement(n, S):
    from indextts.utils import tempo
    assert tempo.out_len(n, S) == R.out_len(n, S) == max(1, (n * 1024 + S // 2) // S)
    assert tempo.frames(n, S) == R.frames(n, S) == (R.out_len(n, S) - 1) // 384 + 2
    if S == 1024:
        assert tempo.out_len(n, S) == n
    # the last frame the overlap-add reads exists, and no frame is left over
    assert (R.out_len(n, S) - 1) // 384 + 1 == R.frames(n, S) - 1


def test_fixed_speed_and_its_refusals():
    from indextts.utils import tempo
    for speed, S in ((0.5, 512), (0.8, 819), (1.0, 1024), (1, 1024), (1.25, 1280), (2.0, 2048), (2, 2048), (np.float32(1.5), 1536)):
        assert tempo.fixed_speed(speed) == S == R.fixed_speed(float(speed))
    for bad in (True, False, "1.0", None, float("nan"), float("inf"), 0.49, 2.01, -1.0, 0, [1.0]):
        with pytest.raises(ValueError, match="speed"):
            tempo.fixed_speed(bad)
    for bad in (511, 2049, 1024.0, True):
        with pytest.raises(ValueError, match="S = "):
            tempo.out_len(100, bad)
    with pytest.raises(ValueError, match="n >= 1"):
        tempo.frames(0, 1024)
    w = tempo.window_table()
    assert w.dtype == torch.float32 and np.array_equal(w.numpy(), R.window32()) and w[0] == 0 and w[384] == 1
    assert np.allclose(w.numpy()[:384].astype(np.float64) + w.numpy()[384:], 1.0, atol=1e-7)       # the two halves sum to one


# ------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("S", [819, 1280])
def test_the_reference_keeps_a_tone_at_its_pitch(S):
    x = R.tone(12000)
    offs = [0] + [f.d for f in R.chain(x, S)]
    y, _ = R.overlap_add(x, S, offs)
    assert y.size == R.out_len(12000, S)

    def peak_hz(v):
        spec = np.abs(np.fft.rfft(v * np.hanning(v.size)))
        return np.argmax(spec) * R.RATE / v.size, R.RATE / v.size

    hz, bin_hz = peak_hz(y)
    assert abs(hz - 200.0) <= bin_hz, (hz, bin_hz)
    resampled = np.interp(np.arange(y.size) * S / 1024.0, np.arange(x.size), x)        # played faster instead: the pitch moves
    assert abs(peak_hz(resampled)[0] - 200.0 * S / 1024) <= bin_hz
    assert abs(np.sqrt(np.mean(y[800:-800] ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)) - 1.0) < 0.02      # and the level stays


@functools.lru_cache(maxsize=None)
def chains():
    return tuple(R.chain(x, S) for (_, S, _), x in zip(R.CASES, R.case_rows()))


def test_the_audit_inputs_are_not_ambiguous():
    """In the reference alone: at most 10 % of the non-silent frames of any input are ambiguous, one long row has none at all, and
    the frames the negative controls need exist."""
    whole = []
    for (n, S, _), ch in zip(R.CASES, chains()):
        assert len(ch) == R.frames(n, S) - 1
        live = [f for f in ch if not f.silent]
        assert sum(f.ambiguous for f in live) <= 0.10 * len(live), (n, S)
        if not any(f.ambiguous for f in live):
            whole.append((n, S))
        if n == 24000:
            assert any(f.silent for f in ch), "a frame inside a gap"
            assert any(f.margin > 4 * f.b and -R.TOL < f.d < R.TOL - 1 for f in live), "a frame whose margin exceeds 4 b"
        assert all(f.d == 0 for f in ch if f.silent)
    assert any(n == 24000 for n, _ in whole), whole
    assert {n for n, _, _ in R.CASES} == {1, 383, 384, 385, 769, 2400, 24000} and {S for _, S, _ in R.CASES} == {512, 819, 1024, 1280, 2048}


def test_the_audit_takes_the_reference_and_refuses_the_controls():
    i = [c[:2] for c in R.CASES].index((24000, 1280))
    x, S, ch = R.case_rows()[i], 1280, chains()[i]
    offs = [0] + [f.d for f in ch]
    assert R.audit(x, S, offs) == []
    f = next(f for f in ch if not f.silent and f.margin > 4 * f.b and -R.TOL < f.d < R.TOL - 1)
    for step in (-1, 1):                                               # one lag moved by one where the margin is large
        moved = list(offs)
        moved[f.k] += step
        assert f.k in [k for k, _ in R.audit(x, S, moved)]
    assert R.audit(x, S, offs, template_at=0)                          # the template taken from p_(k-1) instead of p_(k-1) + HOP
    s = next(f for f in ch if f.silent)
    flipped = list(offs)
    flipped[s.k] = R.choose(np.zeros(2 * R.TOL), reverse_ties=True)    # the tie rule reversed on a silent frame
    assert flipped[s.k] != 0 and (s.k, f"a silent frame at the lag {flipped[s.k]}") in R.audit(x, S, flipped)
    assert R.audit(x, S, offs[:-1]) and R.audit(x, S, [1] + offs[1:])
    y, bound = R.overlap_add(x, S, offs)
    assert R.within(y.astype(np.float32), y, bound + 2.0 ** -24 * np.abs(y))
    assert not R.within(R.overlap_add(x, S, offs, swap_halves=True)[0], y, bound)
    assert not R.within(R.overlap_add(x, S, offs, p_shift=1)[0], y, bound)


# ------------------------------------------------------------------------------------------------------- public surface
def test_the_whole_utterance_calls_take_speed_and_the_streams_refuse_it():
    from indextts.infer import IndexTTS
    for name in ("infer", "infer_fast", "infer_batch", "infer_queue"):
        p = inspect.signature(getattr(IndexTTS, name)).parameters
        assert "speed" in p and p["speed"].default is None and p["speed"].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream", "serve_stream_queue"):
        assert "speed" not in inspect.signature(getattr(IndexTTS, name)).parameters, name
    tts = object.__new__(IndexTTS)
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream"):      # ... nor let it pass for a generation setting
        with pytest.raises(TypeError, match="the streams do not take speed="):
            next(iter(getattr(IndexTTS, name)(tts, None, [], speed=None)))         # (infer_stream's checks run at its first next())
    with pytest.raises(TypeError, match="speed"):
        IndexTTS.serve_stream_queue(tts, lambda: None, speed=1.25)


def test_every_bad_speed_is_a_value_error_before_anything_runs():
    from indextts.infer import IndexTTS
    tts = object.__new__(IndexTTS)                                     # no model, no device: a call that got any further would fail otherwise
    texts = [torch.tensor([1, 2]), torch.tensor([3])]
    for bad in (True, float("nan"), float("inf"), 0.4, 2.5, "fast", [1.0], [1.0, 1.0, 1.0], [1.0, True], [0.8, 3.0], (1.0, float("nan"))):
        for name in ("infer_batch", "infer_queue"):
            with pytest.raises(ValueError, match=name + ".*speed"):
                getattr(IndexTTS, name)(tts, None, texts, speed=bad)
    for bad in (True, float("nan"), 0.4, 2.5, "fast", [1.0], [0.8, 1.25]):
        for name in ("infer", "infer_fast"):
            with pytest.raises(ValueError, match=name + ".*speed"):
                getattr(IndexTTS, name)(tts, "prompt.wav", "text", None, speed=bad)
    assert IndexTTS._check_speed(None, "x", 3) is None and IndexTTS._check_speed(1.0, "x") is None
    assert IndexTTS._check_speed([None, 1.0, 1], "x", 3) is None and IndexTTS._check_speed(1.25, "x") == 1280
    assert IndexTTS._check_speed(0.8, "x", 2) == [819, 819] and IndexTTS._check_speed([0.8, None, 1.0], "x", 3) == [819, None, 1024]


def test_speed_none_runs_nothing_of_the_feature(monkeypatch):
    """infer_batch on host stand-ins for its two stages: with speed None, 1.0 or [None, 1.0] (and by default) it returns their
    waveforms untouched even though constructing a TempoEngine raises; with another speed it reaches for the engine."""
    from indextts import infer as inf

    class Boom:
        def __init__(self, *a, **kw):
            raise AssertionError("TempoEngine was constructed")

    monkeypatch.setattr(inf, "TempoEngine", Boom)
    tts = inf.IndexTTS.__new__(inf.IndexTTS)
    tts.device = torch.device("cpu")
    waves = [torch.arange(5, dtype=torch.float32), torch.zeros(3)]
    tts._batch_tokens = lambda *a, **kw: {"rows": ["codes"]}
    tts._batch_waveforms = lambda st, ev, reuse_prefix: list(waves)
    texts = [torch.tensor([1, 2]), torch.tensor([3])]
    for kw in ({}, {"speed": None}, {"speed": 1.0}, {"speed": 1}, {"speed": [None, 1.0]}, {"speed": [None, None]}):
        got = tts.infer_batch(torch.zeros(1, 100, 8), texts, **kw)
        assert len(got) == 2 and all(g is w for g, w in zip(got, waves))
    assert not hasattr(tts, "_tempo")
    for speed in (0.8, [None, 1.25]):
        with pytest.raises(AssertionError, match="TempoEngine was constructed"):
            tts.infer_batch(torch.zeros(1, 100, 8), texts, speed=speed)
    outs, codes = tts.infer_batch(torch.zeros(1, 100, 8), texts, speed=[1.0, None], return_codes=True)
    assert codes == ["codes"] and all(g is w for g, w in zip(outs, waves))


def test_the_command_lines_take_the_speed():
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    api = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    assert re.search(r'"--speed", type=float, default=None', cli) and "--speed does not apply to --stream" in cli
    assert re.search(r"speed: Optional\[float\] = None", api)
    body = api[api.index("def speed_of"):api.index("POST_FIELDS =")]
    assert body.count("status_code=400") == 2 and "streaming" in body
    assert "speed_of(req, streaming=True)" in api[api.index('@app.post("/tts/stream")'):]
    assert "speed_of(req)" in api[api.index('@app.post("/tts")'):api.index('@app.post("/tts/stream")')]
