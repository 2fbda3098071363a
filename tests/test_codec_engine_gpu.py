"""CodecEngine and the IndexTTS surface of the acoustic tokenizer on the GPU (indextts/vqvae/dvae.py).

On the fixture of the reference class (tests/golden/dvae_small.npz): the device's z within 4 x max |z32 - z64| of the fixture's
float64 z -- both are fp32 evaluations of the same twelve layers in different summation orders, so their errors are of one order,
and 4 is the margin for that (measured on an MI355X: the device's max |z - z64| is 4.00e-7, the fixture's own max |z32 - z64|
3.98e-7, the bound 1.59e-6) -- and the device's codes EQUAL the reference run's on every frame (tests/test_codec_cpu.py has shown every
frame decided).  A ragged batch is bit-equal to each clip alone, in any order.

On the 2-layer full-width synthetic model of tests/test_tempo_infer_gpu.py: audio_codes, synthesize_codes (the waveform of
infer_batch from the codes it returned, bit for bit) and extract_codes."""
import os
import warnings

import numpy as np
import pytest
import torch

import codec_refs as R
import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GREEDY = dict(do_sample=False, repetition_penalty=10.0, num_beams=1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_prompt.wav")


def state_dict():
    return {k: torch.from_numpy(v) for k, v in R.fixture()["sd"].items()}


@pytest.fixture(scope="module")
def engine():
    from indextts.vqvae import CodecEngine
    return CodecEngine(state_dict(), DEV)


@pytest.fixture(scope="module")
def mels():
    fx = R.fixture()
    return [torch.from_numpy(fx[T]["mel"]).to(DEV) for T in R.FRAMES]


@pytest.fixture(scope="module")
def encoded(engine, mels):
    return engine.encode(mels, return_z=True)


def test_the_device_z_and_codes_are_the_reference_class(engine, mels, encoded):
    fx = R.fixture()
    codes, zs = encoded
    tau = R.tau(fx)
    worst = 0.0
    for T, c, z in zip(R.FRAMES, codes, zs):
        assert c.dtype == torch.int64 and tuple(c.shape) == (R.code_count(T),) and tuple(z.shape) == (R.code_count(T), 32)
        worst = max(worst, float(np.max(np.abs(z.cpu().numpy().astype(np.float64) - fx[T]["z64"]))))
    print(f"codec engine | max |z_dev - z64| = {worst:.3e}, the fixture's max |z32 - z64| = {tau:.3e}, bound {4 * tau:.3e}")
    assert worst <= 4 * tau
    for T, c in zip(R.FRAMES, codes):
        assert np.array_equal(c.cpu().numpy(), fx[T]["codes"]), T
    assert engine.num_tokens == 64 and engine.codebook_dim == 32 and engine.channels == 100 and len(engine.layers) == 12


def test_a_ragged_batch_is_each_clip_alone_in_any_order(engine, mels, encoded):
    codes, zs = encoded
    before = engine.launches
    for i, m in enumerate(mels):
        (c,), (z,) = engine.encode([m], return_z=True)
        assert torch.equal(c, codes[i]) and torch.equal(z, zs[i])
    assert engine.launches == before + 13 * len(mels)                               # twelve convolutions and the search, any batch
    order = [6, 0, 5, 2, 4, 1, 3, 6]
    c2, z2 = engine.encode([mels[i] for i in order], return_z=True)
    for k, i in enumerate(order):
        assert torch.equal(c2[k], codes[i]) and torch.equal(z2[k], zs[i])
    assert engine.encode([]) == []
    with pytest.raises(ValueError, match="T = 0"):
        engine.encode([mels[0], torch.zeros(100, 0, device=DEV)])
    with pytest.raises(ValueError, match=r"fp32 tensor \[100, T\]"):
        engine.encode([mels[0].cpu()])
    with pytest.raises(ValueError, match=r"fp32 tensor \[100, T\]"):
        engine.encode([torch.zeros(80, 4, device=DEV)])


# --------------------------------------------------------------------------------------------------- the public surface
@pytest.fixture(scope="module")
def tts():
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    t = IndexTTS.from_weights(cfg, weights.gpt_state_dict(2), weights.bigvgan_state_dict(), device=DEV,
                              precision_config=dict(gpt="fp32", vocoder="fp32"), prompt_frontend="hip")
    assert not hasattr(t, "_codec")
    t.load_tokenizer(state_dict=state_dict())
    return t


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def test_audio_codes_of_waveforms(tts):
    from indextts.vqvae import code_count
    t = np.arange(30000) / 24000.0
    waves = [(0.3 * np.sin(2 * np.pi * 220 * t)).astype(np.float32), (0.2 * np.sin(2 * np.pi * 330 * t[:9000])).astype(np.float32)]
    codes, mels = tts.audio_codes(waves, [24000, 16000])
    for c, m in zip(codes, mels):
        assert m.dim() == 3 and m.shape[:2] == (1, 100) and c.dtype == torch.int64 and c.is_cuda
        assert tuple(c.shape) == (code_count(m.shape[-1]),) and int(c.min()) >= 0 and int(c.max()) < 64
    alone, _ = tts.audio_codes(waves[1:], [16000])
    assert torch.equal(alone[0], codes[1])
    want = tts._codec.encode([m[0].contiguous() for m in mels])
    assert all(torch.equal(a, b) for a, b in zip(want, codes))


def test_synthesize_codes_is_infer_batch_from_its_codes(tts):
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    rng = np.random.default_rng(5)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (12, 5, 17)]
    waves, codes = quiet(tts.infer_batch, cond_mel, texts, max_mel_tokens=48, force_stop=[8, 40, 25], seed=7, return_codes=True, **GREEDY)
    again = quiet(tts.synthesize_codes, cond_mel, texts, codes)
    assert len(again) == 3
    for a, w in zip(again, waves):
        assert a.dtype == torch.float32 and torch.equal(a, w)
    one = quiet(tts.synthesize_codes, cond_mel, texts[1:2], [codes[1].to(DEV)])
    assert torch.equal(one[0], waves[1])


def test_extract_codes_of_the_sample_listed_twice(tts, tmp_path):
    from indextts.vqvae import code_count
    lst = tmp_path / "list.txt"
    lst.write_text(f"{SAMPLE}\tfirst\n{SAMPLE}\tsecond\n", encoding="utf-8")
    recs = tts.extract_codes(str(lst), str(tmp_path / "out"), batch_clips=2)
    assert [r["text"] for r in recs] == ["first", "second"] and recs[0]["codes"] != recs[1]["codes"]
    a, b = (np.load(r["codes"]) for r in recs)
    ma, mb = (np.load(r["mels"]) for r in recs)
    assert a.dtype == np.int64 and a.ndim == 2 and a.shape[0] == 1 and np.array_equal(a, b) and np.array_equal(ma, mb)
    assert ma.dtype == np.float32 and ma.shape[:2] == (1, 100) and a.shape[1] == code_count(ma.shape[2]) > 10
    assert recs[0]["duration"] == recs[1]["duration"] > 0.5
    solo = tts.extract_codes(str(lst), str(tmp_path / "solo"), batch_clips=1)
    assert np.array_equal(np.load(solo[1]["codes"]), a)
