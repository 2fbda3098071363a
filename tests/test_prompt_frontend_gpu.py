"""prompt_frontend="hip" through the public interface (2-layer model, bf16 GPT / fp16 vocoder so that both
front-end engines run): the wav -> mel chain on tests/golden/sample_prompt.wav against the float64 chain, held to the torch fp32
path's own error against that chain; prompt_mels against prompt_mel; what the conditioner and the speaker encoder make of the HIP
mel against what they make of the torch mel; greedy codes under either front-end.

Measured on an MI355X (profiles/prompt_frontend.txt): max |exp(out) - exp(logmel64)| / (exp(logmel64) + 1e-7) is 4.1e-4 for the
HIP chain and 3.3e-4 for the torch fp32 chain (both sit on near-silent bins, where the fp32 resampler's error dominates); the
conditioning latents differ by 2.6e-3 at most (rms 5.7e-4), the speaker embedding by 2.3e-5; the greedy codes are equal."""
import os
import warnings

import numpy as np
import pytest
import torch

import melfront_refs as R
import weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "sample_prompt.wav")
GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)


@pytest.fixture(scope="module")
def tts():
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    return IndexTTS.from_weights(cfg, weights.gpt_state_dict(2), weights.bigvgan_state_dict(), device="cuda:0",
                                 precision_config={"gpt": "bf16", "vocoder": "fp16"}, prompt_frontend="hip")


@pytest.fixture(scope="module")
def torch_mel(tts):
    return tts._mel_torch(*tts._decode(WAV))


def test_chain_against_float64_is_held_to_the_torch_paths_own_error(tts, torch_mel):
    from indextts.utils.feature_extractors import MelSpectrogramFeatures, resample
    planar, sr = tts._decode(WAV)
    mono64 = torch.mean(planar, dim=0, keepdim=True).double()        # (the fp32 channel mean, as both paths form it)
    lin64 = MelSpectrogramFeatures()(resample(mono64, sr, 24000)).exp()[0].numpy()
    assert lin64.dtype == np.float64 and lin64.shape == (100, 511)

    def dist(mel):
        return float((np.abs(np.exp(mel[0].double().cpu().numpy()) - lin64) / (lin64 + 1e-7)).max())

    hip = tts.prompt_mel(WAV)
    assert hip.shape == torch_mel.shape == (1, 100, 511) and hip.is_cuda and hip.dtype == torch.float32
    d_hip, d_torch = dist(hip), dist(torch_mel)
    print(f"chain on sample_prompt.wav against float64, max |d| / (mel64 + 1e-7): hip {d_hip:.3e}, torch fp32 {d_torch:.3e}")
    assert d_hip <= 4 * d_torch, (d_hip, d_torch)
    assert torch.equal(tts._prompt(WAV), hip) and tts._prompt(WAV) is tts.cache_cond_mel      # the path cache, the same bits


def test_prompt_mels_equals_prompt_mel_bit_for_bit(tts):
    a, b = R.wave(2, 20000, 5), R.wave(1, 9001, 6)[0]
    n0 = tts.audio_engine.launches
    three = tts.prompt_mels([WAV, (a, 48000), (torch.from_numpy(b), 16000)])
    assert tts.audio_engine.launches == n0 + 4                        # three rates, one log-mel launch
    alone = [tts.prompt_mel(WAV), tts.prompt_mel(a, 48000), tts.prompt_mel(b, sr=16000)]
    assert [tuple(m.shape) for m in three] == [(1, 100, 511), (1, 100, 40), (1, 100, 53)]
    for x, y in zip(three, alone):
        assert torch.equal(x, y)
    same_rate = tts.prompt_mels([(a, 16000), (b, 16000)])
    assert torch.equal(same_rate[1], three[2]) and tts.audio_engine.launches == n0 + 4 + 6 + 2


def test_a_refused_rate_goes_through_the_torch_path_with_one_warning(tts):
    b = R.wave(1, 9001, 6)
    tts._frontend_warned = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = tts.prompt_mels([(b, 44150), (b, 16000), (b, 44150)])
    assert len([w for w in seen if "prompt_frontend='hip'" in str(w.message)]) == 1
    assert torch.equal(got[0], tts._mel_torch(torch.from_numpy(b), 44150)) and torch.equal(got[0], got[2])
    assert torch.equal(got[1], tts.prompt_mel(b, 16000))


def test_conditioner_and_speaker_encoder_on_the_hip_mel(tts, torch_mel):
    """The tolerance is the one tests/test_frontend_gpu.py grants these engines against their functional forms."""
    assert tts.gpt.conditioner() is not None and tts.bigvgan.speaker_engine() is not None
    hip = tts.prompt_mel(WAV)
    c_hip, c_ref = tts._prompt_conds(hip).float(), tts._prompt_conds(torch_mel).float()
    err = (c_hip - c_ref).abs()
    s_hip, s_ref = tts._prompt_spk(hip).float(), tts._prompt_spk(torch_mel).float()
    s_err = (s_hip - s_ref).abs().max().item()
    print(f"HIP mel against torch mel: conditioning latents max {err.max().item():.3e} rms {err.pow(2).mean().sqrt().item():.3e}; "
          f"speaker embedding max {s_err:.3e} (max |ref| {s_ref.abs().max().item():.3f})")
    assert c_hip.shape == (1, 32, 1280) and err.max().item() < 1e-2 and err.pow(2).mean().sqrt().item() < 2e-3
    assert s_hip.shape == (1, 1, 512) and s_err < 2e-2 * max(1.0, s_ref.abs().max().item())


def test_greedy_codes_equal_under_either_front_end(tts, torch_mel):
    rng = np.random.default_rng(5)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (6, 13, 4)]
    kw = dict(max_mel_tokens=12, force_stop=[7, 5, 9], return_codes=True, **GEN)
    _, c_hip = tts.infer_batch(tts.prompt_mel(WAV), texts, **kw)
    _, c_ref = tts.infer_batch(torch_mel, texts, **kw)
    for i, (x, y) in enumerate(zip(c_hip, c_ref)):
        assert torch.equal(x.long().cpu(), y.long().cpu()), (i, x, y)
