"""Continuous batching with the adapter bank (GPTEngine.decode_refill(voices=...)): an utterance takes its voice -- an adapter id, a
weighted mix, or the base voice -- into whichever slot, and at whichever step, it enters.  2-layer full-width engines, the 3-adapter
bank of tests/refill_voices.py, 2 decode slots, check_every = 4."""
import pytest
import torch

from refill_voices import DEV, GREEDY, Voices, same_up_to_a_tie

pytestmark = pytest.mark.gpu
VOICES6 = [0, 2, -1, {0: .7, 1: .3}, 1, {2: 1.2}]
STOPS = [9, 21, 5, 13, 17, 8, 11, 6]


@pytest.fixture(scope="module")
def vs():
    return Voices()


@pytest.fixture(scope="module")
def alone6(vs):
    """(codes, logits) of the six utterances decoded alone under their voices, fp32: computed once, shared, never changed."""
    m = vs.model(torch.float32)
    return [vs.alone(m, i, STOPS[i], VOICES6[i]) for i in range(6)]


def test_every_utterance_gets_the_codes_it_gets_alone_under_its_voice(vs, alone6):
    """fp32, greedy, 2 slots, 6 utterances with voices [0, 2, -1, {0: .7, 1: .3}, 1, {2: 1.2}], paged cache, joined at once and
    staged: the rule of test_decode_refill_gives_every_row_the_codes_it_gets_alone (equal up to the first near-tie)."""
    m = vs.model(torch.float32)
    assert m.engine.paged
    for staged in (False, True):
        got = vs.queue(m, range(6), STOPS, 2, VOICES6, staged=staged)
        assert m.engine.kv is not None and m.engine._mix_host is not None
        for i in range(6):
            want, lg = alone6[i]
            assert int(got[i][-1]) == m.stop_mel_token and got[i].numel() == STOPS[i] + 1, (staged, i, got[i])
            same_up_to_a_tie(got[i], want, lg, (staged, i))
    # the voices matter: the same utterance under another voice gets other codes
    other = vs.alone(m, 0, STOPS[0], 2)[0]
    assert not torch.equal(other, alone6[0][0])


def test_no_voice_leaks_into_the_next_row_of_a_slot(vs, monkeypatch):
    """Slot 0 serves voice 0, then the base voice, then voice 2 (slot 1 holds one long utterance of voice 1).  The base-voice
    utterance gets the codes the same queue gives it on an engine with no bank -- both in the 7-launch step -- and the voice-2
    utterance the codes of its alone run."""
    monkeypatch.setenv("ITTS_DECODE_MODE", "launch")
    m, plain = vs.model(torch.float32), vs.model(torch.float32, bank=False)
    assert m.engine.decode_mode == plain.engine.decode_mode == "launch"
    voices, stops = [0, 1, -1, 2], [5, 36, 6, 7]
    trace = []
    got = vs.queue(m, range(4), stops, 2, voices, staged=False, trace=trace)
    assert [rows for _, rows, _ in trace] == [[0], [0]]            # both refills entered slot 0
    assert (m.engine.adapter_mix.view(torch.int32)[:, 0::2] == -1).all()     # the slots are idle at the end: every record is empty
    base = vs.queue(plain, range(4), stops, 2, staged=False)
    assert torch.equal(got[2], base[2]), (got[2], base[2])
    assert not torch.equal(got[0], base[0])                          # (voice 0 is not the base voice)
    want, lg = vs.alone(m, 3, stops[3], 2)
    assert got[3].numel() == stops[3] + 1
    same_up_to_a_tie(got[3], want, lg, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_an_id_is_the_one_entry_mix_bit_for_bit(vs, dtype):
    m = vs.model(dtype)
    a = vs.queue(m, range(4), STOPS, 2, [0, 2, -1, 0])
    b = vs.queue(m, range(4), STOPS, 2, [{0: 1.0}, {2: 1.0}, None, {0: 1.0}])
    for i in range(4):
        assert torch.equal(a[i], b[i]), (i, a[i], b[i])


@pytest.mark.parametrize("paged", [True, False])
def test_kernel_join_equals_torch_join_and_staged_equals_joined_at_once(vs, alone6, paged):
    """join="torch" and the itts_refill_join launch: equal codes and equal cache contents after the loop, both cache forms;
    staged and joined-at-once loops give equal greedy codes (the rule of the bank-less test: up to a near-tie)."""
    m = vs.model(torch.float32)
    eng = m.engine
    keep, eng.paged = eng.paged, paged
    try:
        out = {}
        for join in ("torch", "kernel"):
            eng._cap_b = eng._cap_s = 0                       # fresh (zeroed) caches for both runs
            codes = vs.queue(m, range(6), STOPS, 2, VOICES6, staged=False, join=join)
            assert (eng.kv is not None) == paged
            out[join] = (codes, eng.kc.clone(), eng.vc.clone(), eng.adapter_mix.clone(), eng.pad.clone(), eng.row_step0.clone())
        for i in range(6):
            assert torch.equal(out["torch"][0][i], out["kernel"][0][i]), i
        for a, b in zip(out["torch"][1:], out["kernel"][1:]):
            assert torch.equal(a, b)
        assert out["kernel"][1].abs().sum().item() > 0
        staged = vs.queue(m, range(6), STOPS, 2, VOICES6, staged=True)
        for i in range(6):
            same_up_to_a_tie(staged[i], out["kernel"][0][i], alone6[i][1], i)
    finally:
        eng.paged = keep


def test_one_captured_step_serves_every_voice(vs):
    """The graphs captured after the first block of steps are all the queue ever captures, although every slot changes voice."""
    m = vs.model(torch.float32)
    eng = m.engine
    eng._graphs.clear()
    vs.queue(m, range(2), [3, 3], 2, VOICES6)                     # one block of steps, no refill
    n = len(eng._graphs)
    assert n == 1 and all(k[-1][0] == "bank-mix" for k in eng._graphs)
    vs.queue(m, range(6), STOPS, 2, VOICES6)
    vs.queue(m, range(6), STOPS, 2, VOICES6[::-1])
    assert len(eng._graphs) == n
    vs.queue(m, range(4), STOPS, 2, [0, 1, 2, -1])                # ids: the same step
    assert len(eng._graphs) == n


def test_voices_beside_per_row_sampling(vs):
    """Each utterance its own seed and voice (fp32, do_sample, top_k = 5, temperature 0.9, no penalty, top_p = 1: the allowed set is
    the five largest logits).  Every sampled token lies in that set, recomputed from the logits of the utterance run alone under
    its voice and teacher-forced with the sampled codes (a logit within 1e-3 of the fifth counts: another left padding).  Utterances
    4 and 5 share text, voice and seed and enter different slots at different polls: equal codes."""
    m = vs.model(torch.float32)
    voices = [0, 2, -1, {0: .7, 1: .3}, {1: .5, 2: .5}, {1: .5, 2: .5}]
    texts = vs.texts[:4] + [vs.texts[6], vs.texts[6]]
    stops = [2, 6, 14, 2, 7, 7]             # slot 1 takes utterance 4 at step 12, slot 0 utterance 5 at step 20
    seeds = [11, 12, 13, 14, 15, 15]
    rows = [dict(do_sample=True, temperature=0.9, top_k=5, top_p=1.0, repetition_penalty=1.0, seed=s, stream=0) for s in seeds]
    trace = []
    got = vs.queue(m, range(6), stops, 2, voices, settings=rows, texts=texts, trace=trace, max_new=16, staged=False)
    slots = [r for _, rs, _ in trace for r in rs]
    polls = [n for n, rs, _ in trace for _ in rs]
    assert slots[2] != slots[3] and polls[2] != polls[3]           # utterances 4 and 5: another slot and another poll
    assert torch.equal(got[4], got[5]), (got[4], got[5])
    assert len({tuple(got[i].tolist()) for i in range(4)}) == 4
    for i in range(6):
        c = got[i]
        assert c.numel() == stops[i] + 1 and int(c[-1]) == m.stop_mel_token
        lg = vs.forced_logits(m, texts[i], c, voices[i]) / 0.9
        for s in range(stops[i]):                                    # (the last token is the forced stop)
            fifth = torch.topk(lg[s], 5).values[-1].item()
            assert lg[s, int(c[s])].item() >= fifth - 1e-3, (i, s, int(c[s]))


def test_bf16_refilled_rows_track_the_merged_fp32_models(vs):
    """bf16, greedy with force_stop, eager launches so that every step's logits can be read: the logits every token of a refilled row
    was chosen from against the merged single-voice fp32 model, run alone and teacher-forced with the row's codes.  RMS < 4e-2,
    the bound profiles/lora_mix_parity.txt holds infer_batch rows to."""
    m = vs.model(torch.bfloat16)
    eng = m.engine
    voices, stops = [0, 2, {0: .7, 1: .3}, -1, 1], [4, 9, 6, 7, 5]
    steps, trace = [], []
    inner = eng._step_transformer

    def step(B, *a, **k):
        r = inner(B, *a, **k)
        steps.append(eng.logits[:B].float().clone())
        return r
    eng._step_transformer = step
    try:
        got = vs.queue(m, range(5), stops, 2, voices, staged=False, use_graph=False, trace=trace, max_new=16)
    finally:
        del eng._step_transformer
    entered = [(n, r, lg[j].float()) for n, rs, lg in trace for j, r in enumerate(rs)]      # utterances 2, 3, 4 in feed order
    assert len(entered) == 3
    for i, (n, slot, first) in zip((2, 3, 4), entered):
        c = got[i]
        # token 0 from the staged prefill's logits; token s from the step that consumed token s - 1: call n + s - 1 of the loop
        mine = torch.stack([first] + [steps[n + s - 2][slot] for s in range(1, c.numel())]).cpu()
        ref = vs.forced_logits(vs.merged(voices[i]), vs.texts[i], c)
        d = mine - ref
        rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
        print(f"bf16 refilled utterance {i} voice {voices[i]}: rms {rms:.3e} max {mx:.3e}")
        assert rms < 4e-2, (i, rms)


def test_refusals(vs):
    m, plain = vs.model(torch.float32), vs.model(torch.float32, bank=False)
    eng = m.engine
    emb, pad = vs.prefix(m, vs.texts[:2])

    def run(fed_voice, e=eng, **kw):
        e.prefill(emb, pad, 200, **({} if e.bank is None else {"adapter_mix": [0, 1]}))
        launched = []
        e._stage = lambda *a, **k: launched.append(1)              # a refusal comes before anything is staged
        try:
            fed = [(emb[0, int(pad[0]):], 3, None, fed_voice)]
            return e.decode_refill(8, GREEDY, lambda k: [fed.pop()] if fed else [], force_stop=[2, 6], check_every=4, staged=False, **kw)
        finally:
            del e._stage
            assert not launched

    for bad in (3, {0: .2, 1: .2, 2: .2, 3: .2, 4: .2}, {0: .1, 1: .1, 2: .1, 0.5: .1, 7: .1}, [(0, 1.0), 1], "voice"):
        with pytest.raises(ValueError):                              # id >= n; five entries; ...; the id form and the pair form at once
            run(bad, voices=[0, 1])
    with pytest.raises(ValueError, match="holds 3 mixes"):           # wrong length
        run(None, voices=[0, 1, 2])
    with pytest.raises(ValueError, match="prefilled under"):        # not the voices of the prefill
        eng.prefill(emb, pad, 200, adapter_mix=[0, 1])
        eng.decode_refill(8, GREEDY, lambda k: [], voices=[0, 2])
    with pytest.raises(ValueError, match="no adapter bank"):
        run(None, e=plain.engine, voices=[0, 1])
    with pytest.raises(ValueError, match="names a voice"):          # a fed voice in a loop without voices
        run(1, e=plain.engine)
    with pytest.raises(NotImplementedError, match="voices="):
        eng.prefill(emb, pad, 200, adapter_mix=[0, 1])
        eng.decode_refill(8, GREEDY, lambda k: [])
    with pytest.raises(ValueError, match="join"):
        run(None, voices=[0, 1], join="scatter")
    with pytest.raises(NotImplementedError):                         # beams
        eng.prefill(emb, pad, 8, beams=3, adapter_mix=[0, 1])
    with pytest.raises(NotImplementedError):
        m.inference_speech(vs.cond_mel, vs.texts[0][None].to(DEV), adapter_mix=[0], num_beams=3, max_generate_length=4)
    torch.cuda.synchronize()
