"""The PCM output back-end without a GPU (libindextts_out.so, indextts/utils/pcm_out.py): the fourth
library's ABI and refusals through ctypes, the plan and the tap table against feature_extractors.resample, the G.711 restatement
of tests/pcm_out_refs.py pinned by properties over all 65 536 int16 values, the stream planner, the bound exercised on an fp32
stand-in of the kernel's order of operations with every negative control outside it, and the public surface's defaults."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import pcm_out_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_out_library_header_and_table_agree():
    from indextts import _native_out as nato
    hdr = open(os.path.join(ROOT, "include", "indextts_out.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(itto_[a-z0-9_]+)\s*\(", code)))
    assert syms == sorted(nato.EXPORTED_SYMBOLS) == ["itto_abi_version", "itto_last_error", "itto_pcm_out"]
    lib = ctypes.CDLL(nato.LIB_PATH)
    lib.itto_abi_version.restype = ctypes.c_int
    assert lib.itto_abi_version() == nato.ABI_VERSION == 1 == int(re.search(r"#define ITTO_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("SRC_RATE", nato.SRC_RATE), ("WINDOW", nato.WINDOW), ("RUN", nato.RUN)):
        assert int(re.search(rf"#define ITTO_{name} (\d+)", hdr).group(1)) == value
    for name, value in nato.ENCODINGS.items():
        assert int(re.search(rf"#define ITTO_ENC_{name.upper()} (\d+)", hdr).group(1)) == value
    assert nato.MAX_TAP_BYTES == 1 << 20 and "#define ITTO_MAX_TAP_BYTES (1 << 20)" in hdr
    assert ctypes.sizeof(nato.Seg) == 64 and ctypes.sizeof(nato.PcmOutArgs) == 80


def test_the_four_libraries_keep_their_symbols_apart():
    from indextts import _native, _native_audio as nata, _native_out as nato, _native_voice as natv
    for other in (_native, nata, natv):
        assert b"itto_" not in open(other.LIB_PATH, "rb").read()
        assert not any(s.startswith("itto_") for s in other.EXPORTED_SYMBOLS)
    mine = open(nato.LIB_PATH, "rb").read()
    assert b"itto_pcm_out" in mine
    for prefix in (b"itta_", b"ittv_", b"itts_"):
        assert prefix not in mine
    lib = ctypes.CDLL(nato.LIB_PATH)
    for other in (_native, nata, natv):
        for s in other.EXPORTED_SYMBOLS:
            assert not hasattr(lib, s), s


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch


def _args(nato, N=1000, x=FAKE, y=FAKE, kern=FAKE, orig=3, new=1, width=19, taps=41, enc=2, x_elems=None, y_elems=None, seg=None):
    n_out = -(-new * N // orig)
    segs = (nato.Seg * 1)(nato.Seg(*(seg or (0, 0, 0, N, N, 0, n_out, 0))))
    a = nato.PcmOutArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.kern_t = x, N if x_elems is None else x_elems, y, n_out if y_elems is None else y_elems, kern
    a.orig, a.new_, a.width, a.taps, a.encoding, a.n_seg = orig, new, width, taps, enc, 1
    a.segs, a.segs_dev = segs, FAKE
    return a, segs


def test_refusals_through_ctypes():
    from indextts import _native_out as nato
    lib = nato.lib()

    def refused(a, what):
        assert lib.itto_pcm_out(ctypes.byref(a[0]), None) == 1 and what in lib.itto_last_error(), lib.itto_last_error()

    assert lib.itto_pcm_out(None, None) == 1 and b"null argument struct" in lib.itto_last_error()
    refused(_args(nato, x=None), b"null pointer")
    refused(_args(nato, y=None), b"null pointer")
    refused(_args(nato, y=FAKE + 4), b"16-byte aligned")
    refused(_args(nato, x=FAKE + 2), b"4-byte aligned")
    refused(_args(nato, kern=FAKE + 8), b"16-byte aligned")
    # 24000 -> 44101 Hz shares no factor: 44101 phases of 24000 + 2 * 6 taps
    refused(_args(nato, orig=24000, new=44101, width=7, taps=24014), b"above ITTO_MAX_TAP_BYTES")
    refused(_args(nato, orig=2400, new=1, width=14546, taps=31492), b"above the staged window")       # 10 Hz
    refused(_args(nato, taps=40), b"taps must be 2 * width + orig")
    refused(_args(nato, kern=None), b"without a tap table")
    refused(_args(nato, enc=4), b"none of ITTO_ENC_")
    refused(_args(nato, x_elems=999), b"lies outside x")
    refused(_args(nato, y_elems=333), b"lies outside y")
    refused(_args(nato, seg=(0, 2, 0, 1000, 1000, 0, 334, 0), y_elems=400), b"lies outside y")                # y_off not a multiple of 4
    refused(_args(nato, seg=(0, 0, 0, 1000, 1000, 0, 335, 0), y_elems=400), b"past the utterance's end")      # out_len is 334
    refused(_args(nato, seg=(0, 0, 0, 1000, 900, 0, 300, 0)), b"past the utterance's end")                    # more samples than N_total
    # the support of output q is [3 q - 19, 3 q + 22): with 1000 samples of an open utterance, q <= 326 is determined
    refused(_args(nato, seg=(0, 0, 0, 1000, -1, 0, 328, 0)), b"has not arrived")
    refused(_args(nato, seg=(0, 0, 100, 900, -1, 39, 300, 0)), b"has not arrived")     # output 39 reads sample 98 < x0
    a = _args(nato, seg=(0, 0, 0, 1000, -1, 0, 0, 0))                                # nothing to produce: taken, no launch
    assert lib.itto_pcm_out(ctypes.byref(a[0]), None) == 0


# ------------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("rate", [8000, 11025, 16000, 22050, 44100, 48000])
def test_plan_and_table_are_what_resample_builds(rate, monkeypatch):
    from indextts.utils import feature_extractors as fe, pcm_out as po
    seen = {}
    real = fe.F.conv1d

    def spy(x, kern, stride):
        seen["kern"], seen["stride"], seen["pad"] = kern, stride, x.shape[-1]
        return real(x, kern, stride=stride)

    monkeypatch.setattr(fe.F, "conv1d", spy)
    fe.resample(torch.zeros(1, 4000), 24000, rate)
    orig, new, width, taps = po.out_plan(rate)
    assert (orig, new, width, taps) == R.plan(rate) and seen["stride"] == orig and seen["pad"] == 4000 + 2 * width + orig
    t = po.tap_table(rate)
    assert t.dtype == torch.float32 and tuple(t.shape) == (new, taps) and torch.equal(t, seen["kern"][:, 0])
    assert np.array_equal(t.numpy(), R.taps32(rate))
    packed = po.pack_taps(t)
    assert tuple(packed.shape) == (taps, new) and packed.is_contiguous() and torch.equal(packed.t(), t)
    assert po.refusal(rate) is None


def test_plan_of_the_listed_rates():
    from indextts.utils import pcm_out as po
    assert po.out_plan(11025) == (320, 147, 14, 348) and po.out_plan(22050)[:2] == (160, 147) and po.out_plan(22050)[3] == 174
    assert po.out_plan(8000)[:2] == (3, 1) and po.out_plan(48000)[:2] == (1, 2) and po.out_plan(24000) == (1, 1, 0, 0)


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 22050, 44100, 48000, 24000])
def test_out_len_is_the_length_resample_gives(rate):
    from indextts.utils import feature_extractors as fe, pcm_out as po
    orig, new, width, _ = R.plan(rate)
    for n in range(1, 2001):
        # the length resample() cuts to -- its own expression -- and, at a few n, the tensor it returns
        assert po.out_len(n, rate) == R.out_len(n, rate) == int(np.ceil(new * n / orig))
    for n in (1, 2, 319, 320, 321, 1999, 2000):
        assert fe.resample(torch.zeros(1, n), 24000, rate).shape[-1] == po.out_len(n, rate)


def test_output_format_is_validated():
    from indextts.utils import pcm_out as po
    f = po.OutputFormat()
    assert (f.sample_rate, f.encoding, f.wav_tag, f.dtype, f.content_type) == (24000, "pcm16", 1, torch.int16, "audio/L16; rate=24000")
    g = po.OutputFormat(8000, "mulaw")
    assert (g.wav_tag, g.dtype, g.bytes_per_sample, g.content_type) == (7, torch.uint8, 1, "audio/PCMU; rate=8000")
    assert po.OutputFormat(8000, "alaw").wav_tag == 6 and po.OutputFormat(48000, "f32").wav_tag == 3
    assert g == po.OutputFormat(8000, "mulaw") and g != f and len({g, po.OutputFormat(8000, "mulaw")}) == 1
    for bad in (0, -8000, 8000.0, "8000", None, True):
        with pytest.raises(ValueError, match="positive integer"):
            po.OutputFormat(bad)
    with pytest.raises(ValueError, match="tap table"):
        po.OutputFormat(44101)
    with pytest.raises(ValueError, match="window"):
        po.OutputFormat(10)
    with pytest.raises(ValueError, match="encoding"):
        po.OutputFormat(8000, "opus")
    with pytest.raises(AttributeError):
        g.sample_rate = 16000


# ----------------------------------------------------------------------------------------------------------------- G.711
ALL16 = np.arange(-32768, 32768, dtype=np.int64)


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_restatement_properties_over_every_int16(law):
    enc, dec = (R.mulaw_encode, R.mulaw_decode) if law == "mulaw" else (R.alaw_encode, R.alaw_decode)
    clip = R.MU_CLIP if law == "mulaw" else 32767
    codes = enc(ALL16)
    assert codes.dtype == np.uint8 and len(np.unique(codes)) == 256
    levels = np.unique(np.abs(dec(np.arange(256))))                                   # the representable magnitudes
    assert levels.size == 128 and (np.diff(levels) > 0).all()
    back = dec(codes)
    # decode(encode(s)) has the sign of s (mu-law's -1 .. -3 land on its negative zero; A-law has no zero level: 0 -> +8) ...
    nz = ALL16 != 0
    assert (back[ALL16 > 0] > 0 if law == "alaw" else back[ALL16 > 0] >= 0).all() and (back[ALL16 < 0] <= 0).all()
    assert (np.sign(back) == np.sign(ALL16))[nz & (np.abs(back) > 0)].all() and back[ALL16 == 0] == (8 if law == "alaw" else 0)
    # ... and is A representable level nearest to min(|s|, clip) -- everywhere but in the first eighth of a segment's first cell.
    # There the Recommendation's own decision levels (the segment boundaries) give the cell's level L although the top level of
    # the segment below, at L - 3 w / 4 for the new step w, is nearer: G.711 is a midpoint quantiser per cell, and at a segment
    # boundary the cells double.  That is 2 * sum(w / 8) = 508 values for mu-law (steps 16 .. 1024), 498 for A-law (steps
    # 32 .. 1024; a negative value sits one further into its cell).  The exceptions are pinned exactly, not tolerated loosely.
    want = np.minimum(np.abs(ALL16), clip)
    nearest = np.abs(levels[None, :] - want[:, None]).min(1)
    err = np.abs(np.abs(back) - want)
    c_inv = (~codes if law == "mulaw" else codes ^ 0x55).astype(np.int64)
    seg, mant = (c_inv >> 4) & 7, c_inv & 0xF
    step = (8 << seg) if law == "mulaw" else np.where(seg == 0, 16, 8 << seg)
    assert (2 * err <= step).all()                                     # never more than half the cell's step away
    off = err != nearest
    assert int(off.sum()) == (508 if law == "mulaw" else 498)
    first = 1 if law == "mulaw" else 2                                 # (A-law's segments 0 and 1 share one step)
    assert (mant[off] == 0).all() and (seg[off] >= first).all() and (np.abs(back)[off] > want[off]).all()
    assert (8 * (np.abs(back)[off] - want[off]) > 3 * step[off]).all() and (err[off] - nearest[off] <= step[off] // 4).all()
    # every code is a fixed point, except mu-law's negative zero
    c = np.arange(256)
    again = enc(dec(c))
    ok = again == c
    if law == "mulaw":
        assert dec(0x7F) == 0 and not ok[0x7F] and again[0x7F] == 0xFF
        ok[0x7F] = True
    assert ok.all()
    # monotone in s: through the decoder, the code's value never falls as s rises
    assert (np.diff(back) >= 0).all()
    assert law != "mulaw" or (enc(0) == 0xFF and enc(-1) == 0x7F and enc(32767) == 0x80 and enc(-32768) == 0x00)
    assert law != "alaw" or (enc(0) == 0xD5 and enc(-1) == 0x55 and enc(32767) == 0xAA and enc(-32768) == 0x2A)


def test_g711_controls_differ():
    s = ALL16[::7]
    assert (R.mulaw_encode(s, bias=128) != R.mulaw_encode(s)).sum() > 100           # (4 units of bias: the values near a cell's edge)
    small = np.arange(-200, 200)
    assert (R.mulaw_encode(small, bias=128) != R.mulaw_encode(small)).mean() > 0.3
    assert (R.alaw_encode(s, xor=0) != R.alaw_encode(s)).all()
    x = R.gauss(1000)
    assert (R.pcm16_of(x, "nearest") != R.pcm16_of(x)).mean() > 0.3


# --------------------------------------------------------------------------------------------------------- stream planner
@pytest.mark.parametrize("rate", R.RATES)
def test_stream_planner_tiles_the_outputs_once_in_order(rate):
    from indextts.utils import pcm_out as po
    orig, new, width, taps = po.out_plan(rate)
    rng = np.random.default_rng(rate)
    for trial in range(40):
        N = int(rng.integers(1, 3000))
        sizes = {0: [1] * N, 1: [max(1, taps // 3)] * N, 2: None}.get(trial % 4)
        sp, left, nxt, hi_seen, i = po.StreamPlan(rate), N, 0, 0, 0
        while True:
            c = min(left, sizes[i] if sizes else int(rng.choice([0, 1, 2, 7, 255, 256, 257, 1000])))
            i += 1
            left -= c
            last = left == 0
            before = sp.x0
            p = sp.advance(c, last)
            assert p["j0"] == nxt and p["j1"] >= p["j0"] and p["x0"] == before and p["x0"] + p["n_in"] == N - left
            nxt = p["j1"]
            if p["j1"] > p["j0"]:
                # the support of what is emitted is among the samples handed over; before the end it has all ARRIVED, and the
                # next output's has not
                lo = (p["j0"] // new) * orig - width
                hi = ((p["j1"] - 1) // new) * orig + width + orig
                assert max(lo, 0) >= p["x0"]
                if not last:
                    assert hi <= N - left and p["j1"] % new == 0 and (p["j1"] // new) * orig + width + orig > N - left
            if not last:
                assert N - left - sp.x0 <= taps + orig and sp.x0 <= max(0, (nxt // new) * orig - width)
            if last:
                break
        assert nxt == po.out_len(N, rate)
        with pytest.raises(ValueError, match="last chunk"):
            sp.advance(1, False)


# -------------------------------------------------------------------------------------- bound, stand-in, negative controls
@pytest.mark.parametrize("rate", R.RATES)
def test_standin_sits_within_the_bound_and_the_controls_outside(rate):
    orig, new, width, taps = R.plan(rate)
    worst = 0.0
    for n in R.lengths(rate):
        x, v, b = R.case(rate, n)
        r = R.excess(R.standin32(x, rate), v, b)
        worst = max(worst, r)
        assert r <= 1.0, (rate, n, r)
    x, v, b = R.case(rate, 1000)
    got = R.standin32(x, rate)
    if new > 1:                                                   # (one phase has no neighbour)
        assert R.excess(got, *R.ref64(x, rate, phase_shift=1)) > 1.0
    if rate != 24000:
        assert R.excess(got, *R.ref64(x, rate, width_off=1)) > 1.0
    print(f"rate {rate}: stand-in worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------- public surface
def test_wav_writer_tags_and_payload(tmp_path):
    from indextts.utils.audio import read_audio, write_wav
    for enc, tag, bits, data in (("pcm16", 1, 16, np.array([0, 1, -1, 32767], dtype=np.int16)),
                                 ("f32", 3, 32, np.array([0.0, 0.5, -1.0], dtype=np.float32)),
                                 ("mulaw", 7, 8, np.array([0xFF, 0x7F, 0x80, 1, 2], dtype=np.uint8)),
                                 ("alaw", 6, 8, np.array([0xD5, 0x55, 0xAA], dtype=np.uint8))):
        path = str(tmp_path / f"{enc}.wav")
        write_wav(path, data, 8000, enc)
        raw = open(path, "rb").read()
        assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and len(raw) % 2 == 0
        at = raw.index(b"fmt ")
        size = struct.unpack("<I", raw[at + 4:at + 8])[0]
        fmt = struct.unpack("<HHIIHH", raw[at + 8:at + 24])
        assert fmt == (tag, 1, 8000, 8000 * bits // 8, bits // 8, bits)
        at = raw.index(b"data", at + 8 + size)
        n = struct.unpack("<I", raw[at + 4:at + 8])[0]
        assert raw[at + 8:at + 8 + n] == data.tobytes()
        if enc in ("pcm16", "f32"):
            back, sr = read_audio(path)
            assert sr == 8000 and np.allclose(back, data / (32768.0 if enc == "pcm16" else 1.0))
    with pytest.raises(ValueError, match="encoding"):
        write_wav(str(tmp_path / "x.wav"), np.zeros(3, dtype=np.int16), 8000, "opus")


def test_every_public_call_takes_output_and_defaults_to_none():
    from indextts.infer import IndexTTS
    for name in ("infer", "infer_fast", "infer_batch", "infer_queue", "stream_utterance", "stream_batch", "stream_queue", "infer_stream",
                 "serve_stream_queue"):
        p = inspect.signature(getattr(IndexTTS, name)).parameters
        assert "output" in p and p["output"].default is None and p["output"].kind is inspect.Parameter.KEYWORD_ONLY, name
    from indextts.utils.pcm_out import OutputFormat
    tts = object.__new__(IndexTTS)
    assert IndexTTS.output_format(tts, 8000, "mulaw") == OutputFormat(8000, "mulaw")
    with pytest.raises(ValueError, match="encoding"):
        IndexTTS.output_format(tts, 8000, "mp3")


def test_the_command_lines_take_rate_and_encoding():
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    api = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    assert re.search(r'"--sample-rate", type=int, default=None', cli) and re.search(r'"--encoding", choices=\(.*"mulaw".*\), default=None', cli)
    for field in ("sample_rate", "encoding"):
        assert re.search(field + r": Optional\[\w+\] = None", api), field
    assert "status_code=400" in api[api.index("def output_of"):api.index("def chunk_bytes")]
    assert "audio/PCMU" in open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "utils", "pcm_out.py")).read()
