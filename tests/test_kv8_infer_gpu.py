"""The FP8 KV cache through the public interface: precision_config={"kv_cache": "fp8"} on IndexTTS.from_weights, calibrate_kv,
infer_batch / infer_queue, the beam refusal, and the 16-bit pool without the key (2-layer synthetic model)."""
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS = 2
GREEDY = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=10.0, num_beams=1)
ROWS = [[11, 22, 33, 44, 55, 66, 77], [66, 77, 88], [101, 202, 303, 404, 505], [9, 8, 7, 6]]
STOPS = [11, 6, 9, 4]


@pytest.fixture(scope="module")
def parts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = LAYERS
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    return cfg, weights.gpt_state_dict(LAYERS), weights.bigvgan_state_dict(), cond_mel


def test_fp8_kv_cache_serves_batch_and_queue(parts, capsys):
    from indextts.infer import IndexTTS
    cfg, sd, bsd, cond_mel = parts
    tts = IndexTTS.from_weights(cfg, sd, bsd, device="cuda:0", precision_config={"gpt": "bf16", "kv_cache": "fp8"})
    assert "kv_cache=e4m3" in capsys.readouterr().out
    eng = tts.gpt.engine
    assert tts.kv_cache_dtype == "fp8" and eng.kv_dtype == "fp8" and eng.weight_dtype is None
    assert torch.equal(eng.kv_scale.cpu(), torch.ones(LAYERS, 2, eng.H))                 # until calibrate_kv is called
    rows = [torch.tensor(r) for r in ROWS]
    sc = tts.calibrate_kv(cond_mel, rows)
    assert tuple(sc.shape) == (LAYERS, 2, eng.H) and not torch.equal(sc.cpu(), torch.ones(LAYERS, 2, eng.H))
    wavs, codes = tts.infer_batch(cond_mel, rows, max_mel_tokens=12, force_stop=STOPS, seed=5, return_codes=True, **GREEDY)
    assert eng.kv.kc.element_size() == 1
    assert len(wavs) == 4 and all(int(c.numel()) <= s for c, s in zip(codes, STOPS))
    for w, c in zip(wavs, codes):
        assert w.numel() == int(c.numel()) * 1024 and torch.isfinite(w.float()).all() and w.float().abs().max().item() > 0
    # per-request sampling settings ride on the same cache
    w2, c2 = tts.infer_batch(cond_mel, rows, max_mel_tokens=12, force_stop=STOPS, seed=5, return_codes=True,
                             sampling=[dict(do_sample=False)] * 4, **GREEDY)
    assert all(torch.equal(a, b) for a, b in zip(codes, c2))
    wq, cq = tts.infer_queue(cond_mel, rows, slots=2, max_mel_tokens=12, force_stop=STOPS, seed=5, return_codes=True, check_every=4,
                             **GREEDY)
    assert len(cq) == 4 and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(codes, cq)), (codes, cq)
    assert all(a.numel() == b.numel() for a, b in zip(wavs, wq))
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        tts.infer_batch(cond_mel, rows, max_mel_tokens=12, seed=5, **dict(GREEDY, num_beams=3))


def test_pool_is_16_bit_without_the_key_and_bad_values_raise(parts, capsys):
    from indextts.infer import IndexTTS
    cfg, sd, bsd, cond_mel = parts
    with pytest.raises(ValueError, match="kv_cache"):
        IndexTTS.from_weights(cfg, sd, bsd, device="cuda:0", precision_config={"gpt": "bf16", "kv_cache": "int8"})
    tts = IndexTTS.from_weights(cfg, sd, bsd, device="cuda:0", precision_config={"gpt": "bf16"})
    assert "kv_cache=auto" in capsys.readouterr().out
    assert tts.kv_cache_dtype is None and tts.gpt.engine.kv_dtype is None and tts.gpt.engine.kv_scale is None
    tts.infer_batch(cond_mel, [torch.tensor(r) for r in ROWS[:2]], max_mel_tokens=6, force_stop=[4, 3], seed=5, **GREEDY)
    assert tts.gpt.engine.kv.kc.dtype == torch.bfloat16 and tts.gpt.engine.kv.kc.element_size() == 2
    with pytest.raises(ValueError, match="FP8"):
        tts.calibrate_kv(cond_mel, [torch.tensor(ROWS[0])])
