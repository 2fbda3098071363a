"""The post= keyword on the GPU (IndexTTS.post_process, indextts/utils/post_wave.py), on the 2-layer
full-width synthetic model of tests/test_pcm_out_infer_gpu.py: four utterances, forced stops after 8 / 40 / 75 / 88 codes, fp32,
greedy.  All of it holds by construction and is asserted bit for bit: post=None changes nothing; post=pp is PostWaveEngine.process
of the post=None samples; post=pp with output=fmt is PcmOutEngine.encode of that; infer_queue likewise.

The synthetic vocoder's samples are not speech; the threshold is laid at each test's own median frame level so that the plan has
frames on both sides of it (what the plan then does is pinned by tests/test_post_wave_engine_gpu.py, not here)."""
import warnings

import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
ENDS, LIMIT, CHUNK = [8, 40, 75, 88], 96, 8


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
    """infer_batch() of the four rows, as it has always been: fp32 waveforms."""
    return quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, **GREEDY)


@pytest.fixture(scope="module")
def pp(tts, whole):
    """Trim at the median frame level of the longest row, pauses capped at 30 ms, -20 dBFS."""
    st = tts._post_engine().frame_stats([whole[3]])[0]
    level = 10.0 * np.log10(np.maximum(st[:-1, 0].astype(np.float64) / 240.0, 1e-30) / 32768.0 ** 2)
    return tts.post_process(trim_db=float(np.clip(np.median(level), -119.0, -1.0)), max_pause_ms=30.0, keep_ms=10.0, target_rms_db=-20.0)


def test_post_none_returns_what_the_call_returned(tts, cond_mel, texts, whole):
    st = quiet(tts._batch_tokens, cond_mel, texts, LIMIT, ENDS, 7, None, lazy_spk=True, **GREEDY)       # the path under infer_batch
    old = tts._batch_waveforms(st, None, reuse_prefix=True)
    again = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, post=None, **GREEDY)
    for a, b, c in zip(whole, old, again):
        assert a.dtype == torch.float32 and a.dim() == 1 and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(TypeError, match="PostProcess"):
        tts.infer_batch(cond_mel, texts, post=dict(trim_db=-45.0))
    with pytest.raises(TypeError, match="the streams do not take post="):
        tts.stream_batch(cond_mel, texts, post=None)


def test_infer_batch_post_is_the_engine_on_its_waveforms(tts, cond_mel, texts, whole, pp):
    got = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, post=pp, **GREEDY)
    plans = []
    want = tts._post_engine().process(whole, pp, plans_out=plans)
    for g, w, src in zip(got, want, whole):
        assert g.dtype == torch.float32 and g.dim() == 1 and torch.equal(g, w)
    assert all(p.gain != 1.0 for p in plans)                                                # it did something: the level at least
    print("post_wave infer | kept samples per row", [(p.n_out, int(w.numel()), len(p.pieces), round(p.gain, 4)) for p, w in zip(plans, whole)])


def test_post_composes_with_output(tts, cond_mel, texts, whole, pp):
    fmt = tts.output_format(8000, "mulaw")
    got = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, post=pp, output=fmt, **GREEDY)
    want = tts._out_engine().encode(tts._post_engine().process(whole, pp), fmt)
    for g, w in zip(got, want):
        assert g.dtype == torch.uint8 and torch.equal(g, w)


def test_infer_queue_post_and_output(tts, cond_mel, texts, pp):
    fmt = tts.output_format(8000, "mulaw")
    kw = dict(slots=2, max_mel_tokens=LIMIT, force_stop=ENDS, seed=7, check_every=CHUNK, **GREEDY)
    plain = quiet(tts.infer_queue, cond_mel, texts, **kw)
    none = quiet(tts.infer_queue, cond_mel, texts, post=None, **kw)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    finished = tts._post_engine().process(plain, pp)
    for g, w in zip(quiet(tts.infer_queue, cond_mel, texts, post=pp, **kw), finished):
        assert torch.equal(g, w)
    for g, w in zip(quiet(tts.infer_queue, cond_mel, texts, post=pp, output=fmt, **kw), tts._out_engine().encode(finished, fmt)):
        assert g.dtype == torch.uint8 and torch.equal(g, w)
