"""Voice extraction on the GPU (GPTEngine.extract_lora, IndexTTS.voice_from_checkpoint / add_voice_from_checkpoint; DESIGN.md
section 4.21) on the 2-layer full-width model of the bank tests: voices from refill_voices.make_factors with ranks (4, 8, 16),
checkpoints from merged_state(...) stored as fp16, the way train.py stores them.

(a) The device extraction and the float64 helper (tests/voice_extract_ref.py, explicit difference, same probe) agree on r and on the
    PRODUCTS A^T B^T (the factors are not unique), within the kernel's fp32 bound propagated through the c columns of Q: the result
    is P = Q (D^T Q)^T cut to rank r; the last product D^T Q (reduction length K) is within (K + 2) 2^-24 |D|^T |Q| per element,
    and an error E of it enters P as Q E^T:  |P_device - P_ref| <= (K + 2) 2^-24 |Q| (|Q|^T |D|) per element, no further factor.
    The line printed per target carries the ratio with five decimals.
(b) Two extractions of one checkpoint are bit-equal.
(c) fp32 engine, a bank of the three extracted voices: d_extract = max |logits(extracted bank) - logits(bank of the true factors)|
    over a prefill and 4 decode steps is at most 2 d_merge, d_merge = max |logits(true-factor bank row) - logits(an engine built from
    the fp16 merged checkpoint)| (2: logits are not linear in the difference).  Both go to profiles/voice_extract.txt (`-s`).
(d) add_voice_from_checkpoint on a pool returns the next id, infer_batch(adapter_ids=[id, -1]) runs, and the base row is bit-equal
    to the same call before the voice was added.
(e) tp._generate(...) with a bank still raises, as test_voice_pool_gpu.py pins."""
import numpy as np
import pytest
import torch

import voice_extract_ref as R
import weights
from fp64_check import check
from refill_voices import DEV, Voices, make_factors, make_model, merged_state

pytestmark = pytest.mark.gpu
CODES = torch.tensor([100, 2000, 37, 4100, 512])


def fp16_checkpoint(sd, bank, voice):
    return {k: v.to(torch.float16) for k, v in merged_state(sd, bank, {voice: 1.0}).items()}


@pytest.fixture(scope="module")
def V():
    return Voices()


@pytest.fixture(scope="module")
def base_model(V):
    return make_model(V.sd, torch.float32)


@pytest.fixture(scope="module")
def extracted(V, base_model):
    """Per voice: (checkpoint, (adapters, scaling, report))."""
    out = []
    for v in range(3):
        ck = fp16_checkpoint(V.sd, V.bank, v)
        out.append((ck, base_model.engine.extract_lora(ck)))
    return out


def test_extraction_agrees_with_the_fp64_helper(V, extracted):
    from indextts.gpt.voice_extract import target_keys
    keys = target_keys(2)
    for v, (ck, (adapters, scaling, report)) in enumerate(extracted):
        rank = (4, 8, 16)[v]
        assert scaling == 1.0 and sorted(adapters) == sorted(keys) == sorted(report)
        for key in keys[:4] if v else keys:                    # every target of voice 0, the first layer's four of the others
            D = ck[key + ".weight"].double() - V.sd[key + ".weight"].double()
            K, N = D.shape
            Ar, Br, rep = R.extract_ref(D, index=keys.index(key))
            A, B = adapters[key]
            assert report[key]["r"] == rep["r"] == rank == A.shape[0] and tuple(A.shape) == (rank, K) and tuple(B.shape) == (N, rank)
            assert abs(report[key]["ratio"] - rep["ratio"]) <= 1e-2 * rep["ratio"]
            Q = rep["q"].abs()                                 # the c columns an error of the last product travels through
            bound = (K + 2) * 2.0 ** -24 * (Q @ (Q.t() @ D.abs()))
            what = f"extract voice {v} (r={rank}) {key} [{K}x{N}] ratio {rep['ratio']:.0f}"
            print(f"fp64 | case | {what} | {check(what, A.double().t() @ B.double().t(), Ar.t() @ Br.t(), bound):.5f}")


def test_two_extractions_are_bit_equal(V, base_model, extracted):
    ck, (adapters, _, report) = extracted[1]
    again, _, report2 = base_model.engine.extract_lora(ck)
    assert report == report2 and sorted(again) == sorted(adapters)
    for key, (A, B) in adapters.items():
        assert torch.equal(A, again[key][0]) and torch.equal(B, again[key][1]), key


def test_engine_parity_of_the_extracted_bank(V, extracted):
    m_true = V.model(torch.float32)                            # the bank of the true factors
    m_ext = make_model(V.sd, torch.float32).attach_lora_bank([(ad, sc) for _, (ad, sc, _) in extracted])
    text = V.texts[3]
    d_extract = d_merge = 0.0
    for v in range(3):
        lt = V.forced_logits(m_true, text, CODES, voice=v)
        le = V.forced_logits(m_ext, text, CODES, voice=v)
        lm = V.forced_logits(make_model(extracted[v][0], torch.float32), text, CODES)
        assert lt.shape == le.shape == lm.shape and lt.shape[0] == CODES.numel()
        d_extract = max(d_extract, float((le - lt).abs().max()))
        d_merge = max(d_merge, float((lm - lt).abs().max()))
    print(f"voice_extract | engine parity fp32, 2 layers, ranks (4, 8, 16), prefill + 4 steps | d_extract {d_extract:.3e} | d_merge {d_merge:.3e}")
    assert d_extract <= 2 * d_merge


GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)


def test_public_calls(V, tmp_path):
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    tp = IndexTTS.from_weights(cfg, V.sd, weights.bigvgan_state_dict(), device="cuda:0", precision_config={"gpt": "fp32", "vocoder": "fp32"})
    four = make_factors(V.sd, (4, 8, 16, 8), (2.0, 1.0, 0.5, 1.5), seed=15)
    rng = np.random.default_rng(5)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (9, 6)]
    path = tmp_path / "gpt_finetuned.pth"
    torch.save({"model": fp16_checkpoint(V.sd, four, 3)}, path)
    with pytest.raises(ValueError, match="no voice pool is attached"):
        tp.add_voice_from_checkpoint(str(path))
    assert tp.attach_voice_pool(four[:3], slots=2) == [0, 1, 2]
    with pytest.raises(TypeError, match="returns the pool id"):
        tp.add_voice_from_checkpoint(str(path), return_report=True)
    kw = dict(max_mel_tokens=20, force_stop=[7, 5], return_codes=True, **GEN)
    wav0, codes0 = tp.infer_batch(V.cond_mel, texts, adapter_ids=[0, -1], **kw)
    assert tp.add_voice_from_checkpoint(str(path)) == 3
    wav1, codes1 = tp.infer_batch(V.cond_mel, texts, adapter_ids=[3, -1], **kw)
    assert torch.equal(codes0[1].cpu(), codes1[1].cpu()) and torch.equal(wav0[1].cpu(), wav1[1].cpu())     # the base row
    assert not torch.equal(codes0[0].cpu(), codes1[0].cpu()) or not torch.equal(wav0[0].cpu(), wav1[0].cpu())
    adapters, scaling = tp.voice_from_checkpoint(fp16_checkpoint(V.sd, four, 3))                           # a bare state dict
    assert scaling == 1.0 and all(A.shape[0] == 8 for A, _ in adapters.values()) and len(adapters) == 8
    with pytest.raises(NotImplementedError, match="infer / infer_fast with an adapter bank"):
        tp._generate(None, None, GEN, 20)
    tp.detach_voice_pool()
