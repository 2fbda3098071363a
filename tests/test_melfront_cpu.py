"""The prompt audio front-end without a GPU (libindextts_audio.so, indextts/utils/audio_engine.py):
the third library's ABI and refusals through ctypes, the host tables against feature_extractors.py and torch.stft, the segment
plan, the bounds of tests/melfront_refs.py exercised on an fp32 stand-in of the kernels' order of operations, every negative
control outside them, and the default front-end unchanged."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import melfront_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "sample_prompt.wav")


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_audio_library_header_and_table_agree():
    from indextts import _native_audio as nata
    hdr = open(os.path.join(ROOT, "include", "indextts_audio.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(itta_[a-z0-9_]+)\s*\(", code)))
    assert syms == sorted(nata.EXPORTED_SYMBOLS) == ["itta_abi_version", "itta_last_error", "itta_logmel", "itta_resample"]
    lib = ctypes.CDLL(nata.LIB_PATH)
    lib.itta_abi_version.restype = ctypes.c_int
    assert lib.itta_abi_version() == nata.ABI_VERSION == int(re.search(r"#define ITTA_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("MAX_CHANNELS", nata.MAX_CHANNELS), ("BIN_TILES", nata.BIN_TILES), ("N_BINS", nata.N_BINS)):
        assert int(re.search(rf"#define ITTA_{name} (\d+)", hdr).group(1)) == value
    assert nata.BASIS_ELEMS == 33 * 64 * 2 * 64 * 4 and nata.MAX_TAP_BYTES == 1 << 20
    assert ctypes.sizeof(nata.WaveSeg) == 32 and ctypes.sizeof(nata.MelSeg) == 24


def test_the_other_two_libraries_export_no_audio_symbol():
    from indextts import _native, _native_audio as nata, _native_voice as natv
    assert b"itta_" not in open(_native.LIB_PATH, "rb").read()
    assert b"itta_" not in open(natv.LIB_PATH, "rb").read()
    assert b"itta_logmel" in open(nata.LIB_PATH, "rb").read()
    assert not any(s.startswith("itta_") for s in _native.EXPORTED_SYMBOLS) and len(_native.EXPORTED_SYMBOLS) == 47
    assert natv.EXPORTED_SYMBOLS == ("ittv_abi_version", "ittv_last_error", "ittv_delta_project")


FAKE = 0x10000      # an aligned address that is never read: every case below is refused before any launch


def _resample_args(nata, C=2, N=1000, kern=FAKE, orig=2, new=1, width=13, taps=28, x=FAKE, align=0):
    n_out = -(-new * N // orig)
    segs = (nata.WaveSeg * 1)(nata.WaveSeg(0, 0, C, N, n_out, 0))
    a = nata.ResampleArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.kern = x, C * N, FAKE + align, n_out, kern
    a.orig, a.new_, a.width, a.taps = orig, new, width, taps
    a.segs, a.segs_dev, a.n_seg = segs, FAKE, 1
    return a, segs


def _logmel_args(nata, N=4096, wave=FAKE, basis=FAKE):
    T = 1 + N // 256
    segs = (nata.MelSeg * 1)(nata.MelSeg(0, 0, N, T))
    a = nata.LogmelArgs()
    a.wave, a.wave_elems, a.out, a.out_elems = wave, N, FAKE, 100 * T
    a.basis, a.fb_t, a.mel_rng = basis, FAKE, FAKE
    a.segs, a.segs_dev, a.n_seg = segs, FAKE, 1
    return a, segs


def test_refusals_through_ctypes():
    from indextts import _native_audio as nata
    lib = nata.lib()

    def refused(fn, a, what):
        assert fn(ctypes.byref(a[0]), None) == 1 and what in lib.itta_last_error(), lib.itta_last_error()

    refused(lib.itta_resample, _resample_args(nata, x=None), b"null pointer")
    refused(lib.itta_resample, _resample_args(nata, C=9), b"C=9 channels")
    refused(lib.itta_resample, _resample_args(nata, align=4), b"16-byte aligned")
    # 44101 Hz shares no factor with 24000: 24000 phases of 44101 + 2 * 12 taps
    refused(lib.itta_resample, _resample_args(nata, orig=44101, new=24000, width=12, taps=44125), b"above ITTA_MAX_TAP_BYTES")
    refused(lib.itta_resample, _resample_args(nata, taps=27), b"taps must be 2 * width + orig")
    refused(lib.itta_logmel, _logmel_args(nata, wave=None), b"null pointer")
    refused(lib.itta_logmel, _logmel_args(nata, N=512), b"N=512 samples")
    refused(lib.itta_logmel, _logmel_args(nata, basis=FAKE + 8), b"16-byte aligned")
    assert lib.itta_resample(None, None) == 1 and lib.itta_logmel(None, None) == 1


# ----------------------------------------------------------------------------------------------------------- host tables
@pytest.mark.parametrize("sr", [44100, 48000, 16000, 22050])
def test_tap_table_is_the_kern_resample_builds(sr, monkeypatch):
    from indextts.utils import audio_engine as ae, feature_extractors as fe
    seen = {}
    real = fe.F.conv1d

    def spy(x, kern, stride):
        seen["kern"], seen["stride"] = kern, stride
        return real(x, kern, stride=stride)

    monkeypatch.setattr(fe.F, "conv1d", spy)
    fe.resample(torch.zeros(1, 4000), sr, 24000)
    orig, new, width, taps = ae.resample_plan(sr)
    assert (orig, new, width, taps) == R.resample_plan(sr) and seen["stride"] == orig
    t = ae.tap_table(sr)
    assert t.dtype == torch.float32 and tuple(t.shape) == (new, taps) and torch.equal(t, seen["kern"][:, 0])
    assert np.array_equal(t.numpy(), R.taps32(sr))


def test_tap_table_refuses_a_rate_without_common_factors():
    from indextts.utils import audio_engine as ae
    with pytest.raises(ae.PromptAudioRefused, match="tap table"):
        ae.tap_table(44101)
    with pytest.raises(ae.PromptAudioRefused, match="tap table"):
        ae.segment_plan([(1, 50000)], [44101])
    assert ae.resample_plan(24000) == (1, 1, 0, 0)


def test_bases_reproduce_torch_stft_in_float64():
    from indextts.utils import audio_engine as ae
    c64, s64 = ae.dft_bases64()
    x = torch.from_numpy(R.mel_signal("noise", 4352).astype(np.float64))
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    ref = torch.stft(x[None], 1024, hop_length=256, win_length=1024, window=win, center=True, pad_mode="reflect", normalized=False,
                     onesided=True, return_complex=True)[0].abs().t()                     # [T, 513]
    fr = torch.from_numpy(R.frames_of(x.numpy()))
    got = torch.hypot(fr @ c64, fr @ s64)
    assert got.shape == ref.shape == (18, 513)
    assert (got - ref).abs().max().item() <= 1e-10
    c32, s32 = ae.dft_bases()
    assert torch.equal(c32, c64.float()) and np.array_equal(c32.numpy(), R.bases32()[0]) and np.array_equal(s32.numpy(), R.bases32()[1])


def test_packed_basis_is_the_fragment_order_of_the_header():
    from indextts import _native_audio as nata
    from indextts.utils import audio_engine as ae
    c32, s32 = ae.dft_bases()
    p = ae.pack_basis(c32, s32)
    assert p.numel() == nata.BASIS_ELEMS
    rng = np.random.default_rng(3)
    for nt, ks, cs, g, c, j in zip(rng.integers(0, 33, 200), rng.integers(0, 64, 200), rng.integers(0, 2, 200), rng.integers(0, 4, 200),
                                   rng.integers(0, 16, 200), rng.integers(0, 4, 200)):
        k, f = 16 * ks + 4 * g + j, 16 * nt + c
        want = 0.0 if f > 512 else float((s32 if cs else c32)[k, f])
        assert float(p[(((nt * 64 + ks) * 2 + cs) * 64 + 16 * g + c) * 4 + j]) == want
    assert float(p.reshape(33, -1)[32].abs().sum()) > 0          # bin 512 (Nyquist) lives in the last tile


def test_mel_tables_are_the_filterbank_of_the_torch_path():
    from indextts.utils import audio_engine as ae
    from indextts.utils.feature_extractors import MelSpectrogramFeatures
    fb, fb_t, rng = ae.mel_tables()
    assert torch.equal(fb, MelSpectrogramFeatures().fb) and torch.equal(fb_t, fb.t())
    assert np.array_equal(rng.numpy(), R.mel_ranges(fb.numpy()))
    for m in range(100):
        lo, hi = rng[m].tolist()
        assert float(fb[:lo, m].abs().sum()) == 0 and float(fb[hi:, m].abs().sum()) == 0 and bool((fb[lo:hi, m] > 0).all())
    assert int((fb > 0).sum(1).max()) <= 2                       # two-sparse per bin


def test_segment_plan_and_frame_counts():
    from indextts.utils import audio_engine as ae
    for n in (513, 768, 4095, 4096, 4352, 129600):
        assert ae.frame_count(n) == 1 + n // 256
    for sr in (44100, 48000, 16000, 22050, 24000, 8000):
        orig, new, _, _ = ae.resample_plan(sr)
        for n in (1000, 1029, 1030, 238464):
            assert ae.resampled_len(n, sr) == math.ceil(new * n / orig)
            y = __import__("indextts.utils.feature_extractors", fromlist=["resample"]).resample(torch.zeros(1, n), sr, 24000)
            assert y.shape[-1] == ae.resampled_len(n, sr)
    plan = ae.segment_plan([(2, 238464), (1, 4001), (1, 30000)], [44100, 16000, 44100])
    w = plan["waves"]
    assert [x["n_out"] for x in w] == [129777, 6002, 16327] and [x["T"] for x in w] == [507, 24, 64]
    assert [x["frame_off"] for x in w] == [0, 507, 531] and plan["frames"] == 595
    assert plan["groups"] == {44100: [0, 2], 16000: [1]}
    for a, b in zip(w, w[1:]):
        assert b["x_off"] >= a["x_off"] + a["C"] * a["N"] and b["y_off"] >= a["y_off"] + a["n_out"]
        assert b["x_off"] % 4 == 0 and b["y_off"] % 4 == 0
    assert plan["x_elems"] >= w[-1]["x_off"] + 30000 and plan["y_elems"] >= w[-1]["y_off"] + 16327
    with pytest.raises(ae.PromptAudioRefused, match="9 channels"):
        ae.segment_plan([(9, 4000)], [24000])
    with pytest.raises(ae.PromptAudioRefused, match="reflect"):
        ae.segment_plan([(1, 512)], [24000])
    # whatever the library would refuse, the plan refuses first: IndexTTS sends such a prompt through the torch path
    with pytest.raises(ae.PromptAudioRefused, match="0 channels"):
        ae.segment_plan([(0, 4000)], [24000])
    with pytest.raises(ae.PromptAudioRefused, match="fewer than 2\\^30"):
        ae.segment_plan([(1, 1 << 30)], [24000])
    with pytest.raises(ae.PromptAudioRefused, match="fewer than 2\\^30"):
        ae.segment_plan([(1, 1 << 29)], [8000])
    assert ae.refusal((2, 4000), 44100) is None and "tap table" in ae.refusal((1, 50000), 44101)


# ------------------------------------------------------------------------------------- bounds, stand-in, negative controls
def test_resample_standin_sits_within_the_bound_and_the_control_outside():
    worst, control = 0.0, 0.0
    for label, sr, C, N in R.resample_cases():
        x, y, bound = R.resample_case(sr, C, N)
        r = R.resample_excess(R.resample_standin32(x, sr), y, bound)
        worst = max(worst, r)
        assert r <= 1.0, (label, C, N, r)
        if R.resample_plan(sr)[1] > 1:                           # (2 -> 1 has one phase: there is no neighbour)
            c = R.resample_excess(R.resample_standin32(x, sr, phase_shift=1), y, bound)
            assert c > 1.0, (label, C, N, c)                     # a neighbour's taps: outside on EVERY case with two phases
            control = max(control, c)
    print(f"resample stand-in: worst error / bound {worst:.3f}; neighbour-phase control up to {control:.3e} x the bound")


@pytest.mark.parametrize("kind", R.MEL_SIGNALS)
def test_logmel_standin_sits_within_the_bound(kind):
    for N in R.MEL_LENGTHS:
        x, mel, B = R.mel_case(kind, N)
        out = R.logmel_standin32(x)
        assert out.shape == mel.shape == (100, 1 + N // 256)
        r = R.mel_excess(out, mel, B)
        assert r <= 1.0, (kind, N, r)
        if kind == "zeros":
            assert (out == np.float32(np.log(np.float64(np.float32(1e-7))))).all()


@pytest.mark.parametrize("name", sorted(R.MEL_CONTROLS))
def test_every_logmel_control_exceeds_the_bound_on_some_case(name):
    best = 0.0
    for kind in ("noise", "sine", "impulse0", "impulseN"):
        for N in (768, 4352):
            x, mel, B = R.mel_case(kind, N)
            best = max(best, R.mel_excess(R.logmel_standin32(x, **R.MEL_CONTROLS[name]), mel, B))
    print(f"control '{name}': up to {best:.3e} x the bound")
    assert best > 1.0, (name, best)


# ------------------------------------------------------------------------------------------------- the default front-end
def test_the_torch_front_end_is_unchanged():
    """prompt_frontend="torch" (the default): _prompt() runs the ops it ran before the switch existed, bit for bit."""
    import inspect
    from indextts.infer import IndexTTS
    from indextts.utils.audio import read_audio
    from indextts.utils.feature_extractors import MelSpectrogramFeatures, resample
    assert inspect.signature(IndexTTS.__init__).parameters["prompt_frontend"].default == "torch"
    assert inspect.signature(IndexTTS.from_weights).parameters["prompt_frontend"].default == "torch"
    tts = object.__new__(IndexTTS)
    tts.device, tts.audio_engine, tts.mel_extractor = "cpu", None, MelSpectrogramFeatures()
    tts.cache_cond_mel = tts.cache_audio_prompt = None
    tts._cache_conds = tts._cache_spk = "stale"
    got = IndexTTS._prompt(tts, WAV)
    audio, sr = read_audio(WAV)
    audio = torch.from_numpy(audio.T if audio.ndim > 1 else audio.reshape(1, -1)).float()
    want = MelSpectrogramFeatures()(resample(torch.mean(audio, dim=0, keepdim=True), sr, 24000))
    assert got.shape == (1, 100, 511) and torch.equal(got, want)
    assert tts.cache_audio_prompt == WAV and tts._cache_conds is None and tts._cache_spk is None
    assert IndexTTS._prompt(tts, WAV) is got                                        # the path cache
    assert torch.equal(IndexTTS.prompt_mel(tts, WAV), want)                         # the public form, same ops
    assert torch.equal(IndexTTS.prompt_mel(tts, audio.numpy(), sr), want)
    two = IndexTTS.prompt_mels(tts, [WAV, (audio[:1, :50000], 16000)])
    assert torch.equal(two[0], want) and two[1].shape == (1, 100, 1 + 75000 // 256)
    with pytest.raises(ValueError, match="sample rate"):
        IndexTTS.prompt_mel(tts, audio.numpy())


def test_the_command_lines_take_the_switch():
    cli = open(os.path.join(ROOT, "index-tts-lora_amd", "indextts", "cli.py")).read()
    api = open(os.path.join(ROOT, "index-tts-lora_amd", "api.py")).read()
    for src in (cli, api):
        assert re.search(r'"--prompt-frontend", choices=\("torch", "hip"\), default="torch"', src)
