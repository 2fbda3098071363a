"""Waveform finishing without a GPU (libindextts_post.so, indextts/utils/post_wave.py): the fifth library's
ABI and refusals through ctypes, the host plan against the float64 restatement of tests/post_wave_refs.py on synthetic frame
statistics with its invariants, and the public surface: post=None runs nothing of the feature, the four whole-utterance calls
take the keyword and the streams do not."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import post_wave_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ittp_abi_version", "ittp_frame_stats", "ittp_last_error", "ittp_splice"]


# ------------------------------------------------------------------------------------------------------------------- ABI
def dynamic_symbols(path):
    """The names of the defined global symbols in an ELF64 shared object's .dynsym."""
    raw = open(path, "rb").read()
    assert raw[:5] == b"\x7fELF\x02", "an ELF64 file"
    shoff, = struct.unpack_from("<Q", raw, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", raw, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", raw, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for _, kind, _, _, off, size, link, _, _, entsize in secs:
        if kind != 11:                                           # SHT_DYNSYM
            continue
        str_off = secs[link][4]
        for at in range(off, off + size, entsize):
            name, info, _, shndx, _, _ = struct.unpack_from("<IBBHQQ", raw, at)
            if shndx != 0 and info >> 4 in (1, 2) and name:      # defined, GLOBAL or WEAK
                out.append(raw[str_off + name: raw.index(b"\0", str_off + name)].decode())
    return out


def test_post_library_header_and_table_agree():
    from indextts import _native_post as natp
    hdr = open(os.path.join(ROOT, "include", "indextts_post.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ittp_[a-z0-9_]+)\s*\(", code))) == sorted(natp.EXPORTED_SYMBOLS) == NAMES
    assert sorted(s for s in dynamic_symbols(natp.LIB_PATH) if s.startswith("itt")) == NAMES
    lib = ctypes.CDLL(natp.LIB_PATH)
    lib.ittp_abi_version.restype = ctypes.c_int
    assert lib.ittp_abi_version() == natp.ABI_VERSION == 1 == int(re.search(r"#define ITTP_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("FRAME", 240), ("FADE", 120), ("FRAMES_PER_WG", natp.FRAMES_PER_WG), ("RUN", natp.RUN)):
        assert int(re.search(rf"#define ITTP_{name} (\d+)", hdr).group(1)) == value == getattr(natp, name)
    assert (ctypes.sizeof(natp.Row), ctypes.sizeof(natp.Piece), ctypes.sizeof(natp.OutRow)) == (16, 32, 48)
    assert (ctypes.sizeof(natp.FrameStatsArgs), ctypes.sizeof(natp.SpliceArgs)) == (64, 80)


def test_the_five_libraries_keep_their_symbols_apart():
    from indextts import _native, _native_audio as nata, _native_out as nato, _native_post as natp, _native_voice as natv
    for other in (_native, nata, nato, natv):
        assert not any(s.startswith("ittp_") for s in other.EXPORTED_SYMBOLS)
        assert not any(s.startswith("ittp_") for s in dynamic_symbols(other.LIB_PATH))
    lib = ctypes.CDLL(natp.LIB_PATH)
    for other in (_native, nata, nato, natv):
        for s in other.EXPORTED_SYMBOLS:
            assert not hasattr(lib, s), s
    # the other four tables are what their own tests pin
    assert len(_native.EXPORTED_SYMBOLS) == 47 and nato.EXPORTED_SYMBOLS == ("itto_abi_version", "itto_last_error", "itto_pcm_out")


def test_build_names_the_fifth_library():
    mk = open(os.path.join(ROOT, "index-tts-lora_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(PLIB\)", mk, re.M) and re.search(r"^check:.*\$\(PLIB\)", mk, re.M) and "postwave.hip" in mk
    assert "_native_post.lib()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch


def test_frame_stats_refusals_through_ctypes():
    from indextts import _native_post as natp
    lib = natp.lib()

    def refused(what, rows=((0, 1000),), x=FAKE, stats=FAKE, x_elems=1000, stats_elems=10, stride=5, n_rows=None):
        arr = (natp.Row * len(rows))(*[natp.Row(*r) for r in rows])
        a = natp.FrameStatsArgs()
        a.x, a.x_elems, a.stats, a.stats_elems, a.stat_stride = x, x_elems, stats, stats_elems, stride
        a.n_rows, a.rows, a.rows_dev = len(rows) if n_rows is None else n_rows, arr, FAKE
        assert lib.ittp_frame_stats(ctypes.byref(a), None) == 1 and what in lib.ittp_last_error(), lib.ittp_last_error()

    assert lib.ittp_frame_stats(None, None) == 1 and b"null argument struct" in lib.ittp_last_error()
    refused(b"null pointer", x=None)
    refused(b"16-byte aligned", x=FAKE + 4)
    refused(b"n_rows must be", n_rows=0)
    refused(b"n = 0 samples", rows=((0, 0),))
    refused(b"lies outside x", x_elems=999)
    refused(b"no multiple of 4", rows=((2, 900),))
    refused(b"has 5 frames", stride=4, stats_elems=8)
    refused(b"has 5 frames", stats_elems=9)
    refused(b"has 1 frames", rows=((0, 500), (500, 7)), stride=3, stats_elems=10)          # the second row's slots lie past stats


def splice_args(natp, rows, pieces, x_elems=1000, y_elems=1000, x=FAKE, y=FAKE, ramp=FAKE):
    r = (natp.OutRow * len(rows))(*[natp.OutRow(*v) for v in rows])
    p = (natp.Piece * max(1, len(pieces)))(*[natp.Piece(*v) for v in pieces])
    a = natp.SpliceArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.ramp, a.n_rows, a.n_pieces = x, x_elems, y, y_elems, ramp, len(rows), len(pieces)
    a.rows, a.rows_dev, a.pieces, a.pieces_dev = r, FAKE, p, FAKE
    return a, r, p


def test_splice_refusals_through_ctypes():
    from indextts import _native_post as natp
    lib = natp.lib()

    def refused(what, rows, pieces, **kw):
        a = splice_args(natp, rows, pieces, **kw)
        assert lib.ittp_splice(ctypes.byref(a[0]), None) == 1 and what in lib.ittp_last_error(), lib.ittp_last_error()

    row = (0, 1000, 0, 600, 0, 2, 1.0, 0)
    assert lib.ittp_splice(None, None) == 1 and b"null argument struct" in lib.ittp_last_error()
    refused(b"null pointer", [row], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)], ramp=None)
    refused(b"16-byte aligned", [row], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)], y=FAKE + 8)
    refused(b"lies outside its source row", [row], [(0, 0, 300, 0, 120), (701, 300, 300, 120, 0)])
    refused(b"lies outside its source row", [row], [(-1, 0, 300, 0, 120), (500, 300, 300, 120, 0)])
    refused(b"overlaps the destination", [row], [(0, 0, 300, 0, 120), (500, 299, 301, 120, 0)])
    refused(b"leaves a gap", [row], [(0, 0, 300, 0, 120), (500, 301, 299, 120, 0)])
    refused(b"shorter than its fades", [(0, 1000, 0, 539, 0, 2, 1.0, 0)], [(0, 0, 300, 0, 120), (500, 300, 239, 120, 120)])
    refused(b"each 0 or ITTP_FADE", [row], [(0, 0, 300, 0, 60), (500, 300, 300, 120, 0)])
    refused(b"ends past the row's n_out", [(0, 1000, 0, 500, 0, 2, 1.0, 0)], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)])
    refused(b"cover 300 outputs of n_out = 600", [(0, 1000, 0, 600, 0, 1, 1.0, 0)], [(0, 0, 300, 0, 0)])
    refused(b"lies outside x", [row], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)], x_elems=999)
    refused(b"lies outside y", [row], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)], y_elems=599)
    refused(b"lies outside y", [(0, 1000, 2, 600, 0, 2, 1.0, 0)], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)])   # y_off no multiple of 4
    refused(b"names the pieces", [(0, 1000, 0, 600, 1, 2, 1.0, 0)], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)])
    refused(b"not finite", [(0, 1000, 0, 600, 0, 2, float("nan"), 0)], [(0, 0, 300, 0, 120), (500, 300, 300, 120, 0)])
    a = splice_args(natp, [(0, 1000, 0, 0, 0, 0, 1.0, 0)], [])                            # nothing to produce: taken, no launch
    assert lib.ittp_splice(ctypes.byref(a[0]), None) == 0


# ------------------------------------------------------------------------------------------------------------------ plan
LOUD, QUIET = 240 * 4000.0 ** 2, 240 * 2.0 ** 2       # per-frame sums of squares: -18 dBFS and -84 dBFS


def stats_of(pattern, n=None, peak=9000.0):
    """Synthetic statistics: pattern a string of 'L' (loud) and 'q' (quiet) frames; the last frame holds n - 240 (F - 1) samples."""
    F = len(pattern)
    n = F * 240 if n is None else n
    cnt = np.array([240.0] * (F - 1) + [n - 240.0 * (F - 1)])
    ss = np.array([LOUD if c == "L" else QUIET for c in pattern]) * cnt / 240.0
    pk = np.array([peak if c == "L" else 4.0 for c in pattern])
    return np.stack([ss, pk], 1), n


SETTINGS = [dict(trim_db=-45.0), dict(trim_db=-45.0, max_pause_ms=100.0), dict(trim_db=-45.0, max_pause_ms=100.0, keep_ms=20, target_rms_db=-20.0),
            dict(target_rms_db=-23.0), dict(peak_db=-3.0), dict(trim_db=-45.0, target_rms_db=-6.0, peak_db=-9.0), dict()]
PATTERNS = {
    "no silence": ("L" * 40, None),
    "all silence": ("q" * 40, None),
    "silence at the start": ("q" * 30 + "L" * 20, None),
    "silence at the end": ("L" * 20 + "q" * 30, None),
    "a pause of exactly 100 ms": ("q" * 8 + "L" * 10 + "q" * 10 + "L" * 10 + "q" * 8, None),
    "a pause one frame longer": ("q" * 8 + "L" * 10 + "q" * 11 + "L" * 10 + "q" * 8, None),
    "two long pauses": ("L" * 3 + "q" * 40 + "L" + "q" * 25 + "L" * 2 + "q" * 2, None),
    "n no multiple of 240": ("q" * 8 + "L" * 10 + "q" * 30 + "L" * 10 + "q" * 9, 67 * 240 - 113),
    "a loud partial last frame": ("q" * 12 + "L" * 3, 14 * 240 + 1),
    "n below 240": ("L", 17),
    "n below 240, quiet": ("q", 239),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("kw", SETTINGS, ids=[",".join(f"{k}={v:g}" for k, v in s.items()) or "nothing" for s in SETTINGS])
def test_plan_is_the_restatement_and_keeps_its_invariants(name, kw):
    from indextts.utils import post_wave as pw
    st, n = stats_of(*PATTERNS[name])
    pp = pw.PostProcess(**kw)
    got = pw.plan(st.astype(np.float32), n, pp)
    st = st.astype(np.float32).astype(np.float64)
    pieces, gain, n_out = R.plan64(st[:, 0], st[:, 1], n, **kw)
    assert list(got.pieces) == pieces and got.n_out == n_out, (got, pieces)
    assert abs(got.gain - gain) <= 2.0 ** -23 * gain and float(np.float32(got.gain)) == got.gain      # one ulp of the fp32 it is rounded to
    # invariants: ordered, disjoint, inside the row, tiling the output; every cut end faded, no piece shorter than its fades
    end_src = end_dst = 0
    for k, (src, dst, m, fi, fo) in enumerate(got.pieces):
        assert src >= end_src and dst == end_dst and m >= fi + fo and m >= 1 and src + m <= n
        assert fi == (120 if (k > 0 or src > 0) else 0) and fo == (120 if (k < len(got.pieces) - 1 or src + m < n) else 0)
        end_src, end_dst = src + m, dst + m
    assert end_dst == got.n_out == sum(p[2] for p in got.pieces) <= n
    if pp.ceiling_db is not None:
        assert got.gain * st[:, 1].max() <= 32768.0 * 10.0 ** (pp.ceiling_db / 20.0)
    if "L" not in PATTERNS[name][0] and pp.trim_db is not None:
        assert got == pw.Plan(((0, 0, n, 0, 0),), 1.0, n)                                  # nothing but silence: unchanged
    if pp.trim_db is None:
        assert [p[:3] for p in got.pieces] == [(0, 0, n)]


def test_plan_of_the_named_cases():
    from indextts.utils import post_wave as pw
    pp = pw.PostProcess(trim_db=-45.0, max_pause_ms=100.0)
    exact, _ = stats_of(*PATTERNS["a pause of exactly 100 ms"])
    assert pw.plan(exact, 46 * 240, pp).pieces == ((8 * 240 - 1200, 0, 30 * 240 + 2400, 120, 120),)               # not cut
    longer, _ = stats_of(*PATTERNS["a pause one frame longer"])
    assert pw.plan(longer, 47 * 240, pp).pieces == ((720, 0, 18 * 240 - 720 + 1200, 120, 120), (29 * 240 - 1200, 4800, 10 * 240 + 2400, 120, 120))
    assert pw.plan(longer, 47 * 240, pp).n_out == 47 * 240 - 2 * 720 - 240                 # the ends to 50 ms, the pause to 100 ms
    st, n = stats_of("L", 17)
    short = pw.plan(st, n, pw.PostProcess(trim_db=-45.0, target_rms_db=-18.0, peak_db=0.0))
    assert short.pieces == ((0, 0, 17, 0, 0),) and short.n_out == 17 and abs(short.gain * 4000.0 / (32768.0 * 10 ** (-18 / 20.0)) - 1) < 1e-6
    for bad in (0, -5):
        with pytest.raises(ValueError, match="has no frames"):
            pw.plan(np.zeros((0, 2)), bad, pp)
    with pytest.raises(ValueError, match=r"statistics \[2, 2\]"):
        pw.plan(np.zeros((3, 2)), 300, pp)
    # target alone: the RMS of the loud frames lands on the target; the ceiling of -1 dBFS comes with it
    st, n = stats_of("L" * 10, peak=30000.0)
    free = pw.plan(st, n, pw.PostProcess(target_rms_db=-30.0)).gain
    assert abs(20 * np.log10(free * 4000.0 / 32768.0) + 30.0) < 1e-5
    capped = pw.plan(st, n, pw.PostProcess(target_rms_db=-6.0)).gain
    assert (1 - 2.0 ** -22) * 32768.0 * 10 ** (-1 / 20.0) <= capped * 30000.0 <= 32768.0 * 10 ** (-1 / 20.0)      # under it, by two roundings at most


def test_post_process_is_validated():
    from indextts.utils import post_wave as pw
    p = pw.PostProcess()
    assert (p.trim_db, p.max_pause_ms, p.keep_ms, p.target_rms_db, p.peak_db, p.ceiling_db) == (None, None, 50.0, None, None, None)
    assert pw.PostProcess(target_rms_db=-20).ceiling_db == -1.0 and pw.PostProcess(target_rms_db=-20, peak_db=-3).ceiling_db == -3.0
    assert pw.PostProcess(trim_db=-45) == pw.PostProcess(trim_db=-45.0) and len({pw.PostProcess(trim_db=-45), pw.PostProcess(trim_db=-45.0)}) == 1
    for kw in (dict(trim_db=3), dict(trim_db=float("nan")), dict(trim_db="-45"), dict(trim_db=True), dict(max_pause_ms=100), dict(trim_db=-45, max_pause_ms=9),
               dict(keep_ms=4), dict(keep_ms=None), dict(target_rms_db=1), dict(peak_db=0.5), dict(peak_db=-61)):
        with pytest.raises(ValueError, match="PostProcess"):
            pw.PostProcess(**kw)
    with pytest.raises(AttributeError):
        p.trim_db = -40
    r = pw.ramp_table()
    assert r.dtype == torch.float32 and np.array_equal(r.numpy(), R.ramp32()) and 0 < r[0] < r[60] < r[119] < 1
    assert np.allclose(r.numpy().astype(np.float64) + r.numpy()[::-1], 1.0, atol=1e-7)     # a fade-out and a fade-in are complementary


# ------------------------------------------------------------------------------------------------------- public surface
def test_the_whole_utterance_calls_take_post_and_the_streams_do_not():
    from indextts.infer import IndexTTS
    from indextts.utils.post_wave import PostProcess
    for name in ("infer", "infer_fast", "infer_batch", "infer_queue"):
        p = inspect.signature(getattr(IndexTTS, name)).parameters
        assert "post" in p and p["post"].default is None and p["post"].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream", "serve_stream_queue"):
        assert "post" not in inspect.signature(getattr(IndexTTS, name)).parameters, name
    tts = object.__new__(IndexTTS)
    for name in ("stream_utterance", "stream_batch", "stream_queue", "infer_stream"):      # ... nor let it pass for a generation setting
        with pytest.raises(TypeError, match="the streams do not take post="):
            next(iter(getattr(IndexTTS, name)(tts, None, [], post=None)))          # (infer_stream's checks run at its first next())
    assert IndexTTS.post_process(tts, trim_db=-45, target_rms_db=-20) == PostProcess(trim_db=-45, target_rms_db=-20)
    with pytest.raises(ValueError, match="PostProcess"):
        IndexTTS.post_process(tts, trim_db=5)
    with pytest.raises(TypeError, match="PostProcess"):
        IndexTTS.infer_batch(tts, None, [], post=dict(trim_db=-45))


def test_post_none_runs_nothing_of_the_feature(monkeypatch):
    """infer_batch on host stand-ins for its two stages: with post=None (and by default) it returns their waveforms untouched even
    though constructing a PostWaveEngine raises; with a PostProcess it reaches for the engine."""
    from indextts import infer as inf
    from indextts.utils.post_wave import PostProcess

    class Boom:
        def __init__(self, *a, **kw):
            raise AssertionError("PostWaveEngine was constructed")

    monkeypatch.setattr(inf, "PostWaveEngine", Boom)
    tts = inf.IndexTTS.__new__(inf.IndexTTS)
    tts.device = torch.device("cpu")
    waves = [torch.arange(5, dtype=torch.float32), torch.zeros(3)]
    tts._batch_tokens = lambda *a, **kw: {"rows": ["codes"]}
    tts._batch_waveforms = lambda st, ev, reuse_prefix: list(waves)
    for kw in ({}, {"post": None}):
        got = tts.infer_batch(torch.zeros(1, 100, 8), [torch.tensor([1, 2])], **kw)
        assert len(got) == 2 and all(g is w for g, w in zip(got, waves))
    assert not hasattr(tts, "_post_wave")
    with pytest.raises(AssertionError, match="PostWaveEngine was constructed"):
        tts.infer_batch(torch.zeros(1, 100, 8), [torch.tensor([1, 2])], post=PostProcess(trim_db=-45))


def test_the_command_lines_take_the_settings():
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    api = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    for flag in ("--trim-db", "--max-pause-ms", "--target-rms-db", "--peak-db"):
        assert re.search(rf'"{flag}", type=float, default=None', cli), flag
    for field in ("trim_db", "max_pause_ms", "target_rms_db", "peak_db"):
        assert re.search(field + r": Optional\[float\] = None", api), field
    body = api[api.index("def post_of"):api.index("def chunk_bytes")]
    assert body.count("status_code=400") == 2 and "streaming" in body
    assert "post_of(req, streaming=True)" in api[api.index('@app.post("/tts/stream")'):]
