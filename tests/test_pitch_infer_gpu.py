"""The pitch= keyword on the GPU (indextts/utils/tempo.py), on the 2-layer full-width synthetic model of
tests/test_tempo_infer_gpu.py: three utterances, forced stops after 8 / 40 / 75 codes, fp32, greedy.  What holds by construction is
asserted bit for bit: pitch None and 0 are the call without the keyword; a row without a pitch is the speed= call's row; a row with
one is TempoEngine.shift of the plain call's row alone; infer_queue likewise over its own plain rows (a queued utterance's samples
are not infer_batch's bit for bit -- tests/test_engines_gpu.py holds them to 1e-3 -- so the two are compared through their codes
and lengths); infer(pitch=) is the engine on the plain call's joined sentences.

What the kernel computes is pinned by tests/test_pitch_kernels_gpu.py; that the chain moves a pitch and keeps a duration is shown
here on a pulse train, without the vocoder (the synthetic vocoder's samples are not speech)."""
import warnings

import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
ENDS, LIMIT, CHUNK = [8, 40, 75], 96, 8
PITCH = [3, None, -5]
SPEEDS = [None, 1.25, 1.0]


@pytest.fixture(scope="module")
def tts():
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    return IndexTTS.from_weights(cfg, weights.gpt_state_dict(2), weights.bigvgan_state_dict(), device="cuda:0",
                                 precision_config=dict(gpt="fp32", vocoder="fp32"))


@pytest.fixture(scope="module")
def cond_mel():
    return torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (12, 5, 17)]


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


@pytest.fixture(scope="module")
def whole(tts, cond_mel, texts):
    """infer_batch() of the three rows, as it has always been: (fp32 waveforms, codes)."""
    return quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, return_codes=True, **GREEDY)


def test_pitch_none_and_zero_are_the_call_without_it(tts, cond_mel, texts, whole):
    plain, codes = whole
    before = tts._tempo_engine().launches
    for kw in (dict(pitch=None), dict(pitch=0), dict(pitch=[None, 0, 0.0]), dict(pitch=0, speed=1.0)):
        got, got_codes = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, return_codes=True, **kw, **GREEDY)
        assert [c.tolist() for c in got_codes] == [c.tolist() for c in codes]
        for g, p in zip(got, plain):
            assert g.dtype == torch.float32 and torch.equal(g, p)
    assert tts._tempo_engine().launches == before


def test_infer_batch_pitch_and_speed_per_row(tts, cond_mel, texts, whole):
    from indextts.utils import tempo
    plain, codes = whole
    eng = tts._tempo_engine()
    before = eng.launches
    got, got_codes = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, return_codes=True, pitch=PITCH,
                           speed=SPEEDS, **GREEDY)
    assert eng.launches == before + 3                                   # two of WSOLA, one of the resampler, however many rows
    assert [c.tolist() for c in got_codes] == [c.tolist() for c in codes]
    only_speed = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, speed=SPEEDS, **GREEDY)
    assert torch.equal(got[1], only_speed[1]) and got[1].numel() == tempo.out_len(int(plain[1].numel()), 1280)
    for i in (0, 2):
        s = 1.0 if SPEEDS[i] is None else SPEEDS[i]
        assert got[i].dtype == torch.float32 and got[i].dim() == 1
        assert abs(int(got[i].numel()) - int(plain[i].numel()) / s) <= tempo.HOP, (i, got[i].numel(), plain[i].numel())
        alone = eng.shift([plain[i]], pitch=PITCH[i], speed=SPEEDS[i])[0]
        assert torch.equal(got[i], alone)                               # a row's bits do not depend on the batch
        assert not torch.equal(got[i][: 4096], plain[i][: 4096])        # it did something
        assert torch.isfinite(got[i]).all()
    by_hand = eng.shift(list(plain), pitch=PITCH, speed=SPEEDS)
    for g, w in zip(got, by_hand):
        assert torch.equal(g, w)
    one = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, pitch=-2, **GREEDY)
    for g, w in zip(one, eng.shift(list(plain), pitch=-2)):
        assert torch.equal(g, w)


def test_pitch_then_post_then_output(tts, cond_mel, texts, whole):
    plain, _ = whole
    fmt = tts.output_format(8000, "mulaw")
    pp = tts.post_process(target_rms_db=-20.0)
    got = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, pitch=PITCH, speed=SPEEDS, post=pp, output=fmt, **GREEDY)
    shifted = tts._tempo_engine().shift(list(plain), pitch=PITCH, speed=SPEEDS)
    by_hand = tts._out_engine().encode(tts._post_engine().process(shifted, pp), fmt)
    for g, w in zip(got, by_hand):
        assert g.dtype == torch.uint8 and torch.equal(g, w)


def test_infer_queue_pitch(tts, cond_mel, texts, whole):
    kw = dict(slots=2, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, check_every=CHUNK, **GREEDY)
    plain, codes = quiet(tts.infer_queue, cond_mel, texts, return_codes=True, **kw)
    for a, b in zip(plain, quiet(tts.infer_queue, cond_mel, texts, pitch=[None, 0, None], **kw)):
        assert torch.equal(a, b)
    got, got_codes = quiet(tts.infer_queue, cond_mel, texts, pitch=PITCH, speed=SPEEDS, return_codes=True, **kw)
    assert [c.tolist() for c in got_codes] == [c.tolist() for c in codes]
    for g, w in zip(got, tts._tempo_engine().shift(list(plain), pitch=PITCH, speed=SPEEDS)):
        assert torch.equal(g, w)
    batch = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, pitch=PITCH, speed=SPEEDS, **GREEDY)
    assert [c.tolist() for c in codes] == [c.tolist() for c in whole[1]]                     # the same utterances as the batch's ...
    assert [int(g.numel()) for g in got] == [int(b.numel()) for b in batch]                  # ... at the same lengths


def autocorrelation_hz(v, lo=60, hi=170):
    """The pitch of v at 24 kHz from the peak of its autocorrelation at the lags lo .. hi, parabolic interpolation."""
    v = np.asarray(v, dtype=np.float64)
    spec = np.fft.rfft(v, 2 * v.size)
    ac = np.fft.irfft(spec * np.conj(spec))[: hi + 2]
    k = lo + int(np.argmax(ac[lo: hi + 1]))
    a, b, c = ac[k - 1: k + 2]
    return 24000.0 / (k + 0.5 * (a - c) / (a - 2 * b + c))


def test_a_pulse_train_moves_by_four_semitones_and_keeps_its_length(tts):
    from indextts.utils import tempo
    eng = tts._tempo_engine()
    t = np.arange(24000) / 24000.0
    x = sum(np.cos(2 * np.pi * 200.0 * h * t) for h in range(1, 21)) * 1000.0          # 200 Hz pulses, 20 harmonics: up to 4 kHz
    assert abs(autocorrelation_hz(x) - 200.0) <= 0.02 * 200.0
    wav = torch.from_numpy(x.astype(np.float32)).to(tts.device)
    before = eng.launches
    (y,) = eng.shift([wav], pitch=4)
    assert eng.launches == before + 3
    want = 200.0 * 2.0 ** (4 / 12)
    hz = autocorrelation_hz(y.cpu().numpy()[2000:-2000])
    print(f"pitch chain | 200 Hz pulses at +4 semitones: {hz:.2f} Hz (want {want:.2f}), {y.numel()} samples from {wav.numel()}")
    assert abs(hz - want) <= 0.02 * want
    assert abs(int(y.numel()) - int(wav.numel())) <= tempo.HOP
    (z,) = eng.shift([wav], pitch=-4, speed=1.25)
    assert abs(autocorrelation_hz(z.cpu().numpy()[2000:-2000], lo=60, hi=260) - 200.0 * 2.0 ** (-4 / 12)) <= 0.02 * 200.0 * 2.0 ** (-4 / 12)
    assert abs(int(z.numel()) - wav.numel() / 1.25) <= tempo.HOP


def test_refusals_come_before_any_launch_and_the_streams_refuse(tts, cond_mel, texts):
    eng = tts._tempo_engine()
    before = eng.launches
    for kw, what in ((dict(pitch=13), "pitch = 13"), (dict(pitch=[3, 3]), "2 pitches for 3 utterances"),
                     (dict(pitch=12, speed=0.5), "pitch = 12 semitones at speed = 0.5"), (dict(pitch=[0, None, -12], speed=[1.0, 1.0, 1.5]), "outside")):
        for name in ("infer_batch", "infer_queue"):
            with pytest.raises(ValueError, match=name + ".*" + what):
                getattr(tts, name)(cond_mel, texts, **kw)
    wav = torch.zeros(1000, device=tts.device)
    with pytest.raises(ValueError, match="outside"):
        eng.shift([wav], pitch=-12, speed=1.5)
    with pytest.raises(ValueError, match="fp32 tensor"):
        eng.shift([wav.cpu()], pitch=2)
    assert eng.launches == before
    with pytest.raises(TypeError, match="the streams do not take pitch="):       # TypeError, as for speed=
        tts.stream_batch(cond_mel, texts, pitch=2)
    with pytest.raises(TypeError, match="the streams do not take speed="):
        tts.stream_batch(cond_mel, texts, speed=1.25)


def test_infer_pitch_is_the_engine_on_the_joined_sentences(tts, tmp_path, monkeypatch):
    from indextts.utils.audio import write_pcm16
    t = np.arange(int(24000 * 1.2)) / 24000.0
    prompt = str(tmp_path / "prompt.wav")
    write_pcm16(prompt, (0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype(np.int16), 24000)
    text = "你好世界，今天天气很好。我们去公园散步吧！"
    kw = dict(max_mel_tokens=9, max_text_tokens_per_sentence=8, **GREEDY)
    pieces, vocode = [], tts._vocode

    def recording(*a, **k):
        pieces.append(vocode(*a, **k))
        return pieces[-1]

    monkeypatch.setattr(tts, "_vocode", recording)
    rate, pcm = quiet(tts.infer, prompt, text, None, **kw)
    monkeypatch.setattr(tts, "_vocode", vocode)
    joined = torch.cat(pieces, dim=1).reshape(-1)
    assert rate == 24000 and len(pieces) >= 2
    want = tts._tempo_engine().shift([joined], pitch=2, speed=0.8)[0]
    rate, got = quiet(tts.infer, prompt, text, None, pitch=2, speed=0.8, **kw)
    assert rate == 24000 and got.shape == (want.numel(), 1) and np.array_equal(got[:, 0], want.cpu().type(torch.int16).numpy())
    rate, same = quiet(tts.infer, prompt, text, None, pitch=0, **kw)
    assert np.array_equal(same, pcm)
    rate, fast_plain = quiet(tts.infer_fast, prompt, text, None, **kw)
    rate, fast = quiet(tts.infer_fast, prompt, text, None, pitch=-3, **kw)
    assert abs(fast.shape[0] - fast_plain.shape[0]) <= 384 and not np.array_equal(fast[: 2000], fast_plain[: 2000])
