"""Per-row voice prompts through the public interface: infer_batch / infer_queue / BatchPipeline take cond_mel as a list with one
[1, 100, T_i] prompt per utterance; every utterance comes out as if synthesised alone with its own prompt (2-layer model).

fp32: the conditioner is the functional form per distinct prompt, so a row's greedy codes EQUAL those of the row alone and the
waveforms agree to the tolerance test_infer_queue_equals_utterances_synthesised_one_by_one uses (1e-3 of the int16-range peak).
bf16: the distinct prompts go through ConditionerEngine.batch, whose latents differ from the single-prompt engine's in the last
bits; greedy codes are held to the margin rule of the existing agreement tests (test_engines_gpu.py, test_configs_gpu.py): with
TOL = 4 units of bf16 resolution (2^-8) at the logits' scale, the logits of a row in the batch and alone agree to TOL, and the codes
agree at every step whose top-2 margin of the repetition-penalised scores exceeds 2 TOL, up to the first legitimate flip.
Where TOL comes from: the number format, not the code under test -- the logits are a product of bf16-rounded hidden states, and
"a few units of the storage type's resolution at the values' scale" is the rule test_frontend_gpu.py holds the 16-bit kernels to
(2 to 16 units there; 4 here).  Measured on an MI355X (profiles/prompt_batch.txt; one unit = 2^-8 x max |logit| 4.11 = 1.61e-2):
the prompt list's logits differ from the rows alone by 1.83e-2 (1.1 units); the same batch fed the single-prompt engine's latents --
code older than prompt lists -- differs by 1.16e-2 (0.7 units): batching in bf16 costs most of it, the batched conditioner's
2.5e-3 spread in the latents the rest.  21 (row, step) pairs are decided by the margin rule."""
import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
STOPS = [7, 5, 9, 6]


def make_tts(precision):
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    return IndexTTS.from_weights(cfg, weights.gpt_state_dict(2), weights.bigvgan_state_dict(), device="cuda:0", precision_config=precision)


@pytest.fixture(scope="module")
def tts32():
    return make_tts({"gpt": "fp32", "vocoder": "fp32"})


@pytest.fixture(scope="module")
def tts16():
    return make_tts({"gpt": "bf16", "vocoder": "fp16"})


@pytest.fixture(scope="module")
def prompts():
    """three prompts of different lengths (59 / 33 / 74 subsampled rows), each its own draw"""
    return [torch.from_numpy(synth.uniform(f"in.cond_mel.{i}", (1, 100, T), -6.0, 2.0)).to(DEV) for i, T in enumerate((120, 67, 151))]


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (6, 13, 4, 9, 11, 5)]


def close(w, ref):
    return w.shape == ref.shape and (w - ref).abs().max().item() <= 1e-3 * max(1.0, ref.abs().max().item())


def test_batch_rows_equal_the_rows_alone_fp32(tts32, prompts, texts):
    a, b, c = prompts
    mels = [a, b, a, c]
    outs, codes = tts32.infer_batch(mels, texts[:4], max_mel_tokens=12, force_stop=STOPS, return_codes=True, **GEN)
    assert tts32.gpt.engine.kv_share.item() == 0                  # nothing is shared between the rows' prefixes
    for i in range(4):
        w1, c1 = tts32.infer_batch(mels[i], [texts[i]], max_mel_tokens=12, force_stop=[STOPS[i]], return_codes=True, **GEN)
        assert torch.equal(codes[i].long().cpu(), c1[0].long().cpu()), (i, codes[i], c1[0])
        assert close(outs[i], w1[0]), i
    # the prompt matters: the same text under another prompt is another utterance
    w_other = tts32.infer_batch(b, [texts[0]], max_mel_tokens=12, force_stop=[STOPS[0]], **GEN)[0]
    assert not close(outs[0], w_other)


def _penalised(sc, hist):
    sc = sc.clone()
    ids = torch.tensor(sorted(set(hist)))
    sc[ids] = torch.where(sc[ids] < 0, sc[ids] * 10.0, sc[ids] / 10.0)
    return sc


def test_batch_rows_agree_with_the_rows_alone_bf16(tts16, prompts, texts):
    a, b, c = prompts
    mels = [a, b, a, c]
    tts, eng = tts16, tts16.gpt.engine
    assert tts.gpt.conditioner() is not None
    steps = 10
    sp = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=10.0, seed=0)
    stop_text = tts.cfg.gpt.stop_text_token

    def run(conds, rows):
        L = max(int(t.numel()) for t in rows)
        bh = torch.full((len(rows), L), stop_text, dtype=torch.int32)
        for j, t in enumerate(rows):
            bh[j, : t.numel()] = t
        emb, pad = tts.gpt.prefix_rows(conds, bh)
        eng.prefill(emb, pad, steps + 1, shared_rows=0)
        cd, lg = eng.decode(steps + 1, sp, force_stop=[steps] * len(rows), return_logits=True)
        return cd.cpu(), lg.float().cpu()

    launches0 = tts.gpt.conditioner().launches
    conds, _ = tts._prompt_features(mels, spk=False)
    assert conds.shape == (4, 32, 1280) and torch.equal(conds[0], conds[2]) and not torch.equal(conds[0], conds[1])
    assert tts.gpt.conditioner().launches == 72 and launches0 in (0, 72)          # three distinct prompts, one pass
    cb, lb = run(conds, texts[:4])
    # the yardstick's own noise, printed beside the new path's: the same batch with the SINGLE-prompt engine's latents gathered per
    # row (code that existed before prompt lists) against the rows alone -- what batching alone costs in bf16
    _, lb_old = run(torch.cat([tts._prompt_conds(m) for m in mels], 0), texts[:4])
    decided, worst, worst_old, scale = 0, 0.0, 0.0, 0.0
    for i in range(4):
        c1, l1 = run(tts._prompt_conds(mels[i]), [texts[i]])
        tol = 4 * 2.0 ** -8 * l1.abs().max().item()
        scale = max(scale, l1.abs().max().item())
        worst_old = max(worst_old, (lb_old[:steps, i] - l1[:steps, 0]).abs().max().item())
        hist = [1, 8192]
        for s in range(steps):
            err = (lb[s, i] - l1[s, 0]).abs().max().item()
            worst = max(worst, err)
            assert err < tol, (i, s, err, tol)
            sc = _penalised(l1[s, 0], hist)
            top2 = torch.topk(sc, 2).values
            ta, tb = int(cb[i, s]), int(c1[0, s])
            if (top2[0] - top2[1]).item() > 2 * tol:
                assert ta == tb, (i, s, ta, tb)
                decided += 1
            if ta != tb:
                break                                    # a legitimate flip ends the comparable prefix
            hist.append(ta)
    print(f"bf16 logits, batch against alone, max-abs over 4 rows x {steps} steps (max |logit| {scale:.3f}, one unit 2^-8 x that = "
          f"{2.0 ** -8 * scale:.3e}): prompt list {worst:.3e}; single-prompt latents gathered per row {worst_old:.3e}; decided {decided}")
    assert decided >= 8, decided                         # the margin rule must not make the check vacuous
    # and end to end: waveforms of the right lengths
    outs, codes = tts.infer_batch(mels, texts[:4], max_mel_tokens=12, force_stop=STOPS, return_codes=True, **GEN)
    assert [int(cd.numel()) for cd in codes] == STOPS
    assert all(w.numel() == n * 1024 and torch.isfinite(w).all() for w, n in zip(outs, STOPS))


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_a_list_of_one_prompt_is_that_prompt(which, tts32, tts16, prompts, texts):
    tts = tts32 if which == "fp32" else tts16
    a = prompts[0]
    kw = dict(max_mel_tokens=12, force_stop=STOPS, return_codes=True, **GEN)
    w1, c1 = tts.infer_batch(a, texts[:4], **kw)
    w4, c4 = tts.infer_batch([a, a, a, a], texts[:4], **kw)
    for i in range(4):
        assert torch.equal(c1[i], c4[i]) and torch.equal(w1[i], w4[i])


def test_queue_of_three_prompts_through_two_slots_fp32(tts32, prompts, texts):
    """6 utterances, 3 prompts, 2 slots: four utterances enter through the refill path with their own prompt's latents."""
    a, b, c = prompts
    mels = [a, b, c, a, b, c]
    stops = [7, 3, 9, 5, 8, 4]
    want = [tts32.infer_batch(mels[i], [texts[i]], max_mel_tokens=12, force_stop=[stops[i]], return_codes=True, **GEN) for i in range(6)]
    outs, codes = tts32.infer_queue(mels, texts, slots=2, max_mel_tokens=12, force_stop=stops, return_codes=True, **GEN)
    for i in range(6):
        assert torch.equal(codes[i].long().cpu(), want[i][1][0].long().cpu()), (i, codes[i], want[i][1][0])
        assert close(outs[i], want[i][0][0]), i
    # the pipeline's stage A / B take the list as infer_batch does
    from indextts.infer import BatchPipeline
    pipe = BatchPipeline(tts32)
    try:
        got = pipe.submit(mels[:4], texts[:4], max_mel_tokens=12, force_stop=stops[:4], **GEN).result()
    finally:
        pipe.close()
    for i in range(4):
        assert close(got[i], want[i][0][0]), i


def test_changing_batch_compositions_keep_the_conditioner_buffers_bounded(tts16, prompts, texts):
    """Three prompt lengths, a new ordered composition with every call: the conditioner keeps a bounded number of buffer sets."""
    a, b, c = prompts
    ce = tts16.gpt.conditioner()
    sets = lambda: sum(isinstance(k[0], tuple) for k in ce._bufs)        # noqa: E731  (the batch sets; single-prompt sets have an int there)
    for mels in ([a, b, c], [c, b, a], [b, a, c], [c, a, b], [a, c, b], [b, c, a]):
        conds, _ = tts16._prompt_features(mels, spk=False)
        assert conds.shape[0] == 3 and sets() <= ce.MAX_UNRETAINED_SETS
    first, _ = tts16._prompt_features([a, b, c], spk=False)
    alone = torch.cat([tts16._prompt_conds(m) for m in (a, b, c)], 0)
    assert (first - alone).abs().max().item() < 5e-3          # the spread bound of test_prompt_batch_engine_gpu.py


def test_queue_bf16_runs_with_a_prompt_per_utterance(tts16, prompts, texts):
    a, b, c = prompts
    stops = [7, 3, 9, 5, 8, 4]
    outs, codes = tts16.infer_queue([a, b, c, a, b, c], texts, slots=2, max_mel_tokens=12, force_stop=stops, return_codes=True, **GEN)
    assert [int(cd.numel()) for cd in codes] == stops
    assert all(w.numel() == n * 1024 and torch.isfinite(w).all() for w, n in zip(outs, stops))


def test_prompt_list_with_per_row_sampling_fp32(tts32, prompts, texts):
    """Rows under their own settings AND their own prompts equal the rows alone (greedy rows, different penalties; the sampled
    row keeps its own seed and draw stream, so it too is reproduced by the row alone)."""
    a, b, c = prompts
    mels = [a, b, a, c]
    sampling = [dict(do_sample=False, repetition_penalty=10.0), dict(do_sample=False, repetition_penalty=2.0),
                dict(do_sample=False, repetition_penalty=1.0), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=11)]
    kw = dict(max_mel_tokens=12, return_codes=True, num_beams=1)
    outs, codes = tts32.infer_batch(mels, texts[:4], force_stop=STOPS, sampling=sampling, **kw)
    for i in range(3):
        w1, c1 = tts32.infer_batch(mels[i], [texts[i]], force_stop=[STOPS[i]], sampling=[sampling[i]], **kw)
        assert torch.equal(codes[i].long().cpu(), c1[0].long().cpu()), i
        assert close(outs[i], w1[0]), i
    assert codes[3].numel() == STOPS[3] and torch.isfinite(outs[3]).all()
    again = tts32.infer_batch(mels, texts[:4], force_stop=STOPS, sampling=sampling, **kw)[1]
    assert all(torch.equal(x, y) for x, y in zip(codes, again))


def test_prompt_list_with_a_lora_bank_fp32(prompts, texts):
    from test_lora_bank_gpu import make_bank
    tts = make_tts({"gpt": "fp32", "vocoder": "fp32"})
    bank, _ = make_bank(weights.gpt_state_dict(2), (8, 16), (2.0, 1.5))
    tts.gpt.attach_lora_bank(bank)
    a, b, c = prompts
    mels, ids = [a, b, a, c], [0, 1, -1, 1]
    kw = dict(max_mel_tokens=12, return_codes=True, **GEN)
    outs, codes = tts.infer_batch(mels, texts[:4], force_stop=STOPS, adapter_ids=ids, **kw)
    for i in range(4):
        w1, c1 = tts.infer_batch(mels[i], [texts[i]], force_stop=[STOPS[i]], adapter_ids=[ids[i]], **kw)
        assert torch.equal(codes[i].long().cpu(), c1[0].long().cpu()), i
        assert close(outs[i], w1[0]), i


def test_errors_come_before_any_launch(tts16, prompts, texts):
    """Without the feature a list fails with AttributeError (`cond_mel.shape` / `_version` of a list); with it, the wrong length
    and beam search are refused before the conditioner, the prefill or the loop launch anything."""
    a, b, c = prompts
    ce = tts16.gpt.conditioner()
    n0 = ce.launches
    ce.launches = -1
    with pytest.raises(ValueError, match="3 prompts for 4 utterances"):
        tts16.infer_batch([a, b, c], texts[:4], max_mel_tokens=12, **GEN)
    with pytest.raises(NotImplementedError, match="prompt per utterance"):
        tts16.infer_batch([a, b, a, c], texts[:4], max_mel_tokens=12, do_sample=False, num_beams=3)
    with pytest.raises(ValueError, match="2 prompts for 6 utterances"):
        tts16.infer_queue([a, b], texts, slots=2, max_mel_tokens=12, **GEN)
    assert ce.launches == -1
    ce.launches = n0
    outs = tts16.infer_batch([a, b], texts[:2], max_mel_tokens=12, force_stop=[4, 5], **GEN)      # the call that fails today
    assert [w.numel() for w in outs] == [4 * 1024, 5 * 1024]
