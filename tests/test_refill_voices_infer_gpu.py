"""infer_queue with voices through the public interface: 5 utterances through 2 slots, each under its own adapter id or mix, against
infer_batch of each utterance alone under the same voice -- the comparison of test_infer_queue_equals_utterances_synthesised_one_by_one
(equal codes, waveforms within 1e-3 of the int16-range peak).  2-layer synthetic model, fp32."""
import numpy as np
import pytest
import torch

import synth
import weights
from refill_voices import DEV, make_factors

pytestmark = pytest.mark.gpu
GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
LENS = [13, 11, 9, 6, 4]
STOPS = [7, 3, 9, 5, 6]


@pytest.fixture(scope="module")
def tts():
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    sd = weights.gpt_state_dict(2)
    t = IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0", precision_config={"gpt": "fp32", "vocoder": "fp32"})
    t.gpt.attach_lora_bank(make_factors(sd, (4, 8, 16), (2.0, 1.0, 0.5)))
    return t


@pytest.fixture(scope="module")
def cond_mel():
    return torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in LENS]


@pytest.mark.parametrize("form,voices", [("adapter_ids", [0, 2, -1, 1, 2]), ("adapter_mix", [{0: .7, 1: .3}, 2, None, {2: 1.2}, {0: .5, 1: .5}])])
def test_infer_queue_with_voices_equals_each_utterance_synthesised_alone(tts, cond_mel, texts, form, voices):
    want = [tts.infer_batch(cond_mel, [texts[i]], max_mel_tokens=20, force_stop=[STOPS[i]], return_codes=True, **{form: [voices[i]]}, **GEN)
            for i in range(5)]
    outs, codes = tts.infer_queue(cond_mel, texts, slots=2, max_mel_tokens=20, force_stop=STOPS, return_codes=True, check_every=4,
                                  **{form: voices}, **GEN)
    for i in range(5):
        w, c = want[i][0][0], want[i][1][0]
        assert torch.equal(codes[i].long().cpu(), c.long().cpu()), (i, codes[i], c)
        assert outs[i].shape == w.shape
        assert (outs[i] - w).abs().max().item() <= 1e-3 * max(1.0, w.abs().max().item()), i


def test_utterances_that_differ_only_in_voice_differ_in_waveform(tts, cond_mel, texts):
    same = [texts[2]] * 4
    outs, codes = tts.infer_queue(cond_mel, same, slots=2, max_mel_tokens=20, force_stop=[8] * 4, return_codes=True, check_every=4,
                                  adapter_mix=[0, 2, None, 0], **GEN)
    assert all(w.numel() == 8 * 1024 and torch.isfinite(w).all() for w in outs)
    assert torch.equal(codes[0], codes[3])                                   # one voice, one text: one result, wherever it ran
    assert (outs[0] - outs[3]).abs().max().item() <= 1e-3 * max(1.0, outs[0].abs().max().item())
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(outs[i], outs[j]), (i, j)


def test_argument_errors_come_before_any_launch(tts, cond_mel, texts):
    eng = tts.gpt.engine
    launched = []
    eng.prefill = lambda *a, **k: launched.append(1)
    try:
        with pytest.raises(NotImplementedError, match="adapter_ids"):
            tts.infer_queue(cond_mel, texts, slots=2, **GEN)
        with pytest.raises(ValueError):
            tts.infer_queue(cond_mel, texts, slots=2, adapter_ids=[0] * 5, adapter_mix=[0] * 5, **GEN)
        with pytest.raises(ValueError):
            tts.infer_queue(cond_mel, texts, slots=2, adapter_ids=[0] * 4, **GEN)
        with pytest.raises(ValueError):
            tts.infer_queue(cond_mel, texts, slots=2, adapter_ids=[0, 1, 2, 3, 0], **GEN)
        with pytest.raises(ValueError):
            tts.infer_queue(cond_mel, texts, slots=2, adapter_mix=[None] * 4 + [{0: .2, 1: .2, 2: .2, 3: .2, 4: .2}], **GEN)
        with pytest.raises(NotImplementedError):
            tts.infer_queue(cond_mel, texts, slots=2, adapter_ids=[0] * 5, **dict(GEN, num_beams=3))
    finally:
        del eng.prefill
    assert not launched
