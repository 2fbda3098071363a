"""The voice pool on the GPU (GPTEngine.attach_lora_pool, IndexTTS.attach_voice_pool): the bank's slots as a cache over a pool of any
size.  The yardstick is always attach_lora_bank itself: an engine whose bank holds, position by position, the voices pool_resident()
reports, run with the ids translated to those positions -- equal tensors, equal codes, equal logits, bit for bit.  2-layer full-width
model of tests/weights.py, voices from refill_voices.make_factors on all four targets."""
import numpy as np
import pytest
import torch

import weights
from refill_voices import DEV, Voices, make_factors, make_model, same_up_to_a_tie

pytestmark = pytest.mark.gpu
RANKS = (4, 8, 16, 4, 16, 8)
SCALES = (2.0, 1.0, 0.5, 1.5, 0.75, 1.25)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def V():
    return Voices()


@pytest.fixture(scope="module")
def six(V):
    return make_factors(V.sd, RANKS, SCALES, seed=11)


@pytest.fixture(scope="module")
def models(V):
    """Per dtype: (the model a pool is attached to, the model a direct bank is attached to)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (make_model(V.sd, DTYPES[name]), make_model(V.sd, DTYPES[name]))
        for m in made[name]:
            m.detach_lora_bank()
        return made[name]
    return get


def pooled(m, voices, slots, rp=16):
    from indextts.gpt.voice_pool import VoicePool
    pool = VoicePool(m.engine, rp)
    ids = [pool.add(ad, sc) for ad, sc in voices]
    assert ids == list(range(len(voices))) and len(pool) == len(voices)
    m.attach_lora_pool(pool, slots)
    return pool


def direct(m, voices, arrangement):
    """attach_lora_bank of the voices in the arrangement a pool engine reports (an empty slot: a voice that names no target)."""
    m.detach_lora_bank()
    m.attach_lora_bank([({}, 1.0) if v is None else voices[v] for v in arrangement])
    return {v: s for s, v in enumerate(arrangement) if v is not None}


def translate(voice, at):
    if voice is None or voice == -1:
        return voice
    return {at[i]: w for i, w in voice.items()} if isinstance(voice, dict) else at[voice]


def batch(V, m, voices, n=4, steps=10):
    """(codes, logits) of the first n texts, greedy, `steps` tokens, every row's logits computed to the end."""
    texts = V.texts[:n]
    bh = torch.full((n, max(int(t.numel()) for t in texts)), m.stop_text_token, dtype=torch.int32)
    for j, t in enumerate(texts):
        bh[j, : t.numel()] = t
    m.engine.skip_finished = False
    c, lg = m.inference_speech(V.cond_mel, bh.to(DEV), do_sample=False, num_beams=1, repetition_penalty=10.0, max_generate_length=steps,
                               return_logits=True, adapter_mix=voices)
    return c.cpu(), lg.cpu()


def bank_tensors(eng):
    return {(i, k): t for i, l in enumerate(eng.layers) for k, t in l.items() if k.startswith("bank_")}


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rp", [16, 48])
def test_images_equal_the_banks_repack_bit_for_bit(V, six, models, dtype, rp):
    mp, md = models(dtype)
    voices = six if rp == 16 else make_factors(V.sd, (8, 40, 16, 24, 36, 4), SCALES, seed=12)
    pooled(mp, voices, 3 if rp == 16 else 2, rp)
    ep = mp.engine
    if rp == 16:
        ep._slots([3, 1, 4], None)
        assert ep.pool_resident() == [3, 1, 4]
    else:                                        # two slots: 3 and 1 first, then 4 takes the least recently used of them
        ep._slots([3, 1], None)
        ep._slots([4], None)
        assert ep.pool_resident() == [4, 1]
    direct(md, voices, ep.pool_resident())
    got, want = bank_tensors(ep), bank_tensors(md.engine)
    assert ep.bank.sig == md.engine.bank.sig and set(got) == set(want) and len(got) == 2 * 4 * 2
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paging_history_moves_no_bit(V, six, models, dtype):
    mp, md = models(dtype)
    pooled(mp, six, 3)
    want_resident = [[0, 1, 2], [3, 1, 4], [0, 1, 5]]
    for voices, resident in zip(([0, 1, 2, -1], [3, 1, 4, 3], [{5: .7, 0: .3}, 5, -1, 1]), want_resident):
        c, lg = batch(V, mp, voices)
        assert mp.engine.pool_resident() == resident
        at = direct(md, six, resident)
        c2, lg2 = batch(V, md, [translate(v, at) for v in voices])
        assert torch.equal(c, c2) and torch.equal(lg, lg2), voices      # the -1 rows too: no stale slot leaks
    st = mp.engine.pool_stats()
    assert st["loads"] == 7 and st["evictions"] == 4 and st["deferrals"] == 0


def test_more_voices_than_a_bank_can_hold(V, models):
    mp, md = models("f32")
    forty = make_factors(V.sd, (4,) * 40, [0.5 + 0.05 * i for i in range(40)], seed=13)
    with pytest.raises(ValueError, match="limit 512"):
        md.attach_lora_bank(forty[:33])                                  # a direct bank stops at 32
    pooled(mp, forty, 4)
    voices = [33, 36, 39, 2]
    c, lg = batch(V, mp, voices)
    at = direct(md, forty, mp.engine.pool_resident())
    c2, lg2 = batch(V, md, [at[v] for v in voices])
    assert torch.equal(c, c2) and torch.equal(lg, lg2)
    base = batch(V, mp, [-1] * 4)[0]
    assert not torch.equal(c, base)                                      # (the voices are audible in the codes)


def test_one_captured_step_serves_every_voice_added_or_removed(V, six, models):
    mp, md = models("f32")
    pool = pooled(mp, six[:5], 3)
    eng = mp.engine
    batch(V, mp, [0, 1, 2, -1])
    n_graphs = len(eng._graphs)
    assert n_graphs >= 1
    batch(V, mp, [3, 4, 3, 1])
    assert len(eng._graphs) == n_graphs
    new = pool.add(*six[5])
    assert new == 5 and len(eng._graphs) == n_graphs
    c = batch(V, mp, [5, -1, 5, 0])[0]
    assert len(eng._graphs) == n_graphs
    at = direct(md, six, eng.pool_resident())
    assert torch.equal(c, batch(V, md, [at[5], -1, at[5], at[0]])[0])
    batch(V, mp, [1, 2, 1, 2])                                          # (a new batch takes the pins over: 5 is free to go)
    pool.remove(5)
    assert len(eng._graphs) == n_graphs and 5 not in eng.pool_resident() and len(pool) == 5
    with pytest.raises(ValueError, match="voices of the pool"):
        batch(V, mp, [5, 0, 0, 0])
    assert pool.add(*six[5]) == 6                                        # an id is never reused


def test_refusals_come_before_any_launch(V, six, models):
    from indextts.gpt.model import UnifiedVoice
    from indextts.gpt.voice_pool import VoicePool
    mp, md = models("bf16")
    pool = pooled(mp, six, 3)
    eng = mp.engine
    launched = []
    eng.prefill = lambda *a, **k: launched.append(1)
    try:
        with pytest.raises(ValueError, match="4 distinct voices.*3 slots"):
            batch(V, mp, [0, 1, 2, 3])
        pool.remove(4)
        with pytest.raises(ValueError, match="voices of the pool"):
            batch(V, mp, [0, 4, 0, 0])
        with pytest.raises(ValueError, match="must be -1 or voices of the pool"):
            eng._voices([0, 4, 0, 0], None, 4)
    finally:
        del eng.prefill
    assert not launched
    big = make_factors(V.sd, (24,), (1.0,), seed=14)[0]
    with pytest.raises(ValueError, match="rank 24"):
        pool.add(*big)
    with pytest.raises(ValueError, match="unknown adapter targets"):
        pool.add({"gpt.h.7.attn.c_attn": big[0]["gpt.h.0.attn.c_attn"]}, 1.0)
    with pytest.raises(ValueError, match="A must be"):
        pool.add({"gpt.h.0.attn.c_attn": six[0][0]["gpt.h.0.mlp.c_proj"]}, 1.0)
    assert len(pool) == 5
    batch(V, mp, [0, 1, 0, -1], steps=3)                                 # the batch in flight pins its voices
    with pytest.raises(ValueError, match="pinned"):
        pool.remove(1)
    spare = VoicePool(md.engine, 16)
    with pytest.raises(ValueError, match="one or the other"):
        mp.attach_lora_pool(spare, 2)                                    # beside a pool
    md.attach_lora_bank(six[:2])
    with pytest.raises(ValueError, match="one or the other"):
        md.attach_lora_pool(spare, 2)                                    # beside a bank
    md.detach_lora_bank()
    md.attach_lora({k: v for k, v in six[0][0].items() if k.endswith("c_proj")}, 1.0)
    with pytest.raises(ValueError, match="single adapters are attached"):
        md.attach_lora_pool(spare, 2)                                    # beside attach_lora
    md.attach_lora(None)
    with pytest.raises(ValueError, match="limit 512"):
        md.attach_lora_pool(spare, 33)
    for kw, err in ((dict(kv_dtype="fp8"), NotImplementedError), (dict(weight_dtype="fp8"), ValueError)):
        m8 = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=2))
        m8.load_state_dict(V.sd)
        m8.to(DEV).to(torch.bfloat16).post_init_gpt2_config(kv_cache=True, **kw)
        with pytest.raises(err, match="attach_lora_pool"):
            m8.attach_lora_pool(spare, 2)


def test_queue_pages_voices_through_two_slots(V, models):
    """6 utterances through 2 decode slots and 2 bank slots; the last one blends two voices, so it can only run alone."""
    mp, md = models("f32")
    four = make_factors(V.sd, (4, 8, 16, 8), (2.0, 1.0, 0.5, 1.5), seed=15)
    pooled(mp, four, 2)
    md.attach_lora_bank(four)
    voices = [0, 1, 2, 0, 3, {1: .5, 2: .5}]
    stops = [7, 3, 9, 5, 12, 6]
    got = V.queue(mp, list(range(6)), stops, 2, voices=voices, check_every=4)
    assert sorted(got) == list(range(6))                                 # nothing lost; V.queue pairs codes with the feed order
    st = mp.engine.pool_stats()
    for i in range(6):
        want, lg = V.alone(md, i, stops[i], voices[i])
        same_up_to_a_tie(got[i], want, lg, ("utt", i))
    assert st["deferrals"] >= 1 and st["evictions"] >= 1
    assert not mp.engine.bank.res.pins                                   # the loop has given every pin back


def test_a_forks_page_ins_leave_the_parent_alone(V, six, models):
    mp, _ = models("f32")
    pooled(mp, six, 3)
    c0 = batch(V, mp, [0, 1, 2, -1])[0]
    before = {k: t.clone() for k, t in bank_tensors(mp.engine).items()}
    r = mp.replica()
    assert r.engine.pool_resident() == [0, 1, 2] and r.engine.bank.res is not mp.engine.bank.res
    batch(V, r, [3, 4, 5, 3])
    assert r.engine.pool_resident() == [3, 4, 5] and mp.engine.pool_resident() == [0, 1, 2]
    now = bank_tensors(mp.engine)
    assert all(torch.equal(before[k], now[k]) and now[k].data_ptr() != bank_tensors(r.engine)[k].data_ptr() for k in before)
    assert torch.equal(batch(V, mp, [0, 1, 2, -1])[0], c0)
    assert mp.engine.pool_stats()["loads"] == 3


# ------------------------------------------------------------------------------------------------------------ public calls
GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
LENS = [13, 11, 9, 6, 4]
STOPS = [7, 3, 9, 5, 6]


@pytest.fixture(scope="module")
def tts_pair():
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    sd = weights.gpt_state_dict(2)
    mk = lambda: IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0",   # noqa: E731
                                       precision_config={"gpt": "fp32", "vocoder": "fp32"})
    return mk(), mk(), make_factors(sd, (4, 8, 16, 8), (2.0, 1.0, 0.5, 1.5), seed=15)


def test_public_calls_take_pool_ids(V, tts_pair):
    tp, td, four = tts_pair
    rng = np.random.default_rng(5)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in LENS]
    assert tp.attach_voice_pool(four[:3], slots=2) == [0, 1, 2]
    assert tp.add_voice(*four[3]) == 3
    eng = tp.gpt.engine
    with pytest.raises(ValueError, match="3 distinct voices.*2 slots"):
        tp.infer_batch(V.cond_mel, texts[:3], max_mel_tokens=20, adapter_ids=[0, 1, 2], **GEN)
    with pytest.raises(NotImplementedError, match="infer / infer_fast with an adapter bank"):
        tp._generate(None, None, GEN, 20)
    _, codes = tp.infer_batch(V.cond_mel, texts[:3], max_mel_tokens=20, force_stop=STOPS[:3], return_codes=True, adapter_ids=[3, 1, 3], **GEN)
    resident = eng.pool_resident()
    assert resident == [3, 1]
    td.gpt.attach_lora_bank([four[v] for v in resident])
    _, want = td.infer_batch(V.cond_mel, texts[:3], max_mel_tokens=20, force_stop=STOPS[:3], return_codes=True, adapter_ids=[0, 1, 0], **GEN)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(codes, want))

    voices = [0, 2, -1, 1, 3]

    def fresh():                                 # the same paging history in front of every run
        tp.detach_voice_pool()
        tp.attach_voice_pool(four, slots=2)
    fresh()
    _, qcodes = tp.infer_queue(V.cond_mel, texts, slots=2, max_mel_tokens=20, force_stop=STOPS, return_codes=True, check_every=4,
                               adapter_ids=voices, **GEN)
    pcm = {}
    for lc in (False, True):
        fresh()
        trace = {}
        ev = list(tp.stream_queue(V.cond_mel, texts, slots=2, chunk_tokens=4, max_mel_tokens=20, seed=1234, force_stop=STOPS,
                                  adapter_ids=voices, latent_cache=lc, _trace=trace, **GEN))
        assert sorted(u for u, _, last in ev if last) == list(range(5))
        for u in range(5):
            assert torch.equal(trace["codes"][u].cpu(), qcodes[u].long().cpu()), (lc, u)
        pcm[lc] = [torch.cat([p for h, p, _ in ev if h == u]) for u in range(5)]
        assert not eng.bank.res.pins and eng.pool_stats()["evictions"] >= 1
    assert all(torch.equal(a, b) for a, b in zip(pcm[False], pcm[True]))
    tp.remove_voice(0)
    with pytest.raises(ValueError, match="voices of the pool"):
        tp.infer_queue(V.cond_mel, texts, slots=2, adapter_ids=voices, **GEN)
    tp.detach_voice_pool()
    assert eng.bank is None


@pytest.mark.parametrize("form,voices", [("adapter_ids", [0, 1, 2, 3, 0, 2]),
                                         ("adapter_mix", [{0: .5, 1: .5}, {2: .7, 3: .3}, 1, {0: .3, 2: .7}, None, 3])])
def test_queues_with_more_decode_slots_than_bank_slots_defer(V, tts_pair, form, voices):
    """4 decode slots over S = 2: the first batch cannot hold the four leading utterances' voices, nor can a closing latent group.
    Every utterance's codes are those of infer_batch of it alone on a directly attached bank of the four voices."""
    tp, td, four = tts_pair
    rng = np.random.default_rng(6)
    lens, stops = [13, 11, 9, 6, 5, 4], [7, 3, 9, 5, 6, 4]
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in lens]
    td.gpt.detach_lora_bank()
    td.gpt.attach_lora_bank(four)
    want = [td.infer_batch(V.cond_mel, [texts[i]], max_mel_tokens=20, force_stop=[stops[i]], return_codes=True, **{form: [voices[i]]}, **GEN)
            for i in range(6)]

    def fresh():
        if tp.gpt.engine.bank is not None:
            tp.detach_voice_pool()
        tp.attach_voice_pool(four, slots=2)
    fresh()
    outs, codes = tp.infer_queue(V.cond_mel, texts, slots=4, max_mel_tokens=20, force_stop=stops, return_codes=True, check_every=4,
                                 **{form: voices}, **GEN)
    eng = tp.gpt.engine
    assert eng._B == (2 if form == "adapter_ids" else 1)                     # the decode slots the voices of the leading rows allowed
    for i in range(6):
        w, c = want[i][0][0], want[i][1][0]
        assert torch.equal(codes[i].long().cpu(), c.long().cpu()), (i, codes[i], c)
        assert outs[i].shape == w.shape and (outs[i] - w).abs().max().item() <= 1e-3 * max(1.0, w.abs().max().item()), i
    assert eng.pool_stats()["evictions"] >= 1 and not eng.bank.res.pins and not eng.bank.res.guards
    fresh()
    trace = {}
    ev = list(tp.stream_queue(V.cond_mel, texts, slots=4, chunk_tokens=4, max_mel_tokens=20, force_stop=stops, _trace=trace,
                              **{form: voices}, **GEN))
    assert sorted(u for u, _, last in ev if last) == list(range(6))
    assert all(torch.equal(trace["codes"][u].cpu(), codes[u].long().cpu()) for u in range(6))
    assert not eng.bank.res.pins and not eng.bank.res.guards
    tp.detach_voice_pool()
