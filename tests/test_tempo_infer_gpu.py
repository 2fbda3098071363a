"""The speed= keyword on the GPU (indextts/utils/tempo.py), on the 2-layer full-width synthetic model of
tests/test_post_wave_infer_gpu.py: four utterances, forced stops after 8 / 40 / 75 / 88 codes, fp32, greedy.  All of it holds by
construction and is asserted bit for bit: the codes are those of the plain call; a row at None or 1.0 is the plain call's row; a
row at another speed is TempoEngine.process of the plain call's row; with post= and output= the result is the three engines
composed by hand in that order; infer_queue likewise; infer(speed=) is the engine on the plain call's joined sentences.

What the kernels compute is pinned by tests/test_tempo_kernels_gpu.py, not here (the synthetic vocoder's samples are not speech)."""
import warnings

import numpy as np
import pytest
import torch

import synth
import tempo_refs as R
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
ENDS, LIMIT, CHUNK = [8, 40, 75, 88], 96, 8
SPEEDS = [0.8, None, 1.25, 1.0]
FIXED = [819, None, 1280, 1024]


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
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (12, 5, 17, 9)]


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


@pytest.fixture(scope="module")
def whole(tts, cond_mel, texts):
    """infer_batch() of the four rows, as it has always been: (fp32 waveforms, codes)."""
    return quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, return_codes=True, **GREEDY)


def test_the_engine_over_a_ragged_list_with_a_speed_per_row(tts, whole):
    from indextts.utils import tempo
    eng = tts._tempo_engine()
    waves = list(whole[0]) + [whole[0][0][:1], torch.zeros(0, device=whole[0][0].device)]
    speeds = FIXED + [2048, 512]
    before, lags = eng.launches, []
    got = eng.process(waves, speeds, offsets_out=lags)
    assert eng.launches == before + 2                                   # two launches, however many rows
    for w, S, g, d in zip(waves, speeds, got, lags):
        if S in (None, 1024) or w.numel() == 0:
            assert g is w and d is None
            continue
        n = int(w.numel())
        assert g.dtype == torch.float32 and g.shape == (tempo.out_len(n, S),) == (R.out_len(n, S),) and d.shape == (R.frames(n, S),)
        alone = eng.process([w], [S])[0]
        assert torch.equal(g, alone)                                    # a row's bits do not depend on the batch
        x = w.cpu().numpy()
        assert R.audit(x, S, d.cpu().numpy()) == []
        want, bound = R.overlap_add(x, S, d.cpu().numpy())
        assert R.within(g.cpu().numpy(), want, bound)
    assert eng.process([], []) == [] and eng.launches == before + 2 + 2 * 3
    with pytest.raises(ValueError, match="speeds for"):
        eng.process(waves, FIXED)
    with pytest.raises(ValueError, match="S = "):
        eng.process(waves[:1], [0.8])
    with pytest.raises(ValueError, match="fp32 tensor"):
        eng.process([waves[0].cpu()], [819])


def test_infer_batch_speed_per_row(tts, cond_mel, texts, whole):
    from indextts.utils import tempo
    plain, codes = whole
    got, got_codes = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, return_codes=True, speed=SPEEDS, **GREEDY)
    assert [c.tolist() for c in got_codes] == [c.tolist() for c in codes]
    want = tts._tempo_engine().process(list(plain), FIXED)
    for i, (g, w, p) in enumerate(zip(got, want, plain)):
        assert g.dtype == torch.float32 and g.dim() == 1 and torch.equal(g, w)
        if FIXED[i] in (None, 1024):
            assert torch.equal(g, p)
        else:
            assert g.numel() == tempo.out_len(int(p.numel()), FIXED[i]) != p.numel()
    one = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, speed=1.25, **GREEDY)
    for g, w in zip(one, tts._tempo_engine().process(list(plain), [1280] * 4)):
        assert torch.equal(g, w)
    for kw in (dict(speed=None), dict(speed=1.0), dict(speed=[None, 1.0, None, 1])):
        for g, p in zip(quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, **kw, **GREEDY), plain):
            assert torch.equal(g, p)
    with pytest.raises(ValueError, match="infer_batch.*3 speeds for 4 utterances"):
        tts.infer_batch(cond_mel, texts, speed=[1.0, 1.0, 1.0])
    with pytest.raises(TypeError, match="the streams do not take speed="):
        tts.stream_batch(cond_mel, texts, speed=1.25)


def test_speed_then_post_then_output(tts, cond_mel, texts, whole):
    plain, _ = whole
    fmt = tts.output_format(8000, "mulaw")
    pp = tts.post_process(target_rms_db=-20.0)
    got = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, speed=SPEEDS, post=pp, output=fmt, **GREEDY)
    by_hand = tts._out_engine().encode(tts._post_engine().process(tts._tempo_engine().process(list(plain), FIXED), pp), fmt)
    for g, w in zip(got, by_hand):
        assert g.dtype == torch.uint8 and torch.equal(g, w)
    assert [int(g.numel()) for g in got] != [int(g.numel()) for g in tts._out_engine().encode(list(plain), fmt)]       # it did something


def test_infer_queue_speed(tts, cond_mel, texts):
    fmt = tts.output_format(8000, "mulaw")
    pp = tts.post_process(target_rms_db=-20.0)
    kw = dict(slots=2, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, check_every=CHUNK, **GREEDY)
    plain, codes = quiet(tts.infer_queue, cond_mel, texts, return_codes=True, **kw)
    for a, b in zip(plain, quiet(tts.infer_queue, cond_mel, texts, speed=[None, 1.0, None, None], **kw)):
        assert torch.equal(a, b)
    at_speed = tts._tempo_engine().process(list(plain), FIXED)
    got, got_codes = quiet(tts.infer_queue, cond_mel, texts, speed=SPEEDS, return_codes=True, **kw)
    assert [c.tolist() for c in got_codes] == [c.tolist() for c in codes]
    for g, w in zip(got, at_speed):
        assert torch.equal(g, w)
    by_hand = tts._out_engine().encode(tts._post_engine().process(at_speed, pp), fmt)
    for g, w in zip(quiet(tts.infer_queue, cond_mel, texts, speed=SPEEDS, post=pp, output=fmt, **kw), by_hand):
        assert g.dtype == torch.uint8 and torch.equal(g, w)


def test_infer_speed_is_the_engine_on_the_joined_sentences(tts, tmp_path, monkeypatch):
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
    assert rate == 24000 and len(pieces) >= 2 and np.array_equal(pcm[:, 0], joined.cpu().type(torch.int16).numpy())
    want = tts._tempo_engine().process([joined], [819])[0]
    rate, slow = quiet(tts.infer, prompt, text, None, speed=0.8, **kw)
    assert rate == 24000 and slow.shape == (R.out_len(joined.numel(), 819), 1)
    assert np.array_equal(slow[:, 0], want.cpu().type(torch.int16).numpy())
    rate, same = quiet(tts.infer, prompt, text, None, speed=1.0, **kw)
    assert np.array_equal(same, pcm)
    rate, fast = quiet(tts.infer_fast, prompt, text, None, speed=1.25, **kw)
    rate, fast_plain = quiet(tts.infer_fast, prompt, text, None, **kw)
    assert fast.shape[0] == R.out_len(fast_plain.shape[0], 1280)
