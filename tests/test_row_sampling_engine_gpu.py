"""Per-row sampling settings through the engine and the public interface: GPTEngine.decode / decode_refill with a list of
settings, IndexTTS.infer_batch(sampling=[...]).  A 2-layer full-width engine in bf16.

The transformer treats the rows of a batch independently, and a row's draw is addressed by (its seed, its stream, its own step):
so row i of a per-row loop must reproduce, exactly, row i of a scalar-parameter loop over the same batch under row i's settings."""
import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = (1 << 33) + 4321
STEPS = 12
GREEDY = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0)
ROWS4 = [dict(GREEDY, repetition_penalty=10.0),
         dict(do_sample=True, temperature=0.7, top_k=30, top_p=0.8, repetition_penalty=10.0),
         dict(do_sample=True, temperature=1.2, top_k=5, top_p=1.0, repetition_penalty=1.0),
         dict(do_sample=True, temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=10.0)]


@pytest.fixture(scope="module")
def model():
    from indextts.gpt.model import UnifiedVoice
    m = UnifiedVoice(**dict(weights.reference_config()["gpt"], layers=2))
    m.load_state_dict(weights.gpt_state_dict(2))
    m.to(DEV).to(torch.bfloat16).post_init_gpt2_config(kv_cache=True)
    return m


@pytest.fixture(scope="module")
def cond_mel():
    return torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)


def prefix(m, conds, texts):
    L = max(int(t.numel()) for t in texts)
    bh = torch.full((len(texts), L), m.stop_text_token, dtype=torch.int32)
    for j, t in enumerate(texts):
        bh[j, : t.numel()] = t
    return m.prefix_rows(conds, bh)


def test_decode_with_a_list_gives_every_row_its_scalar_run(model, cond_mel):
    """B = 4, 12 tokens, rows {greedy} {T 0.7, k 30, p 0.8, rep 10} {T 1.2, k 5, p 1.0, rep 1} {k 1}, stream = row index, the seed of
    the scalar runs: row i equals row i of the scalar-parameter decode of the same batch under row i's settings (four scalar runs),
    graph-replayed and eagerly launched; a second assignment of settings replays the one captured per-row step."""
    m, eng = model, model.engine
    rng = np.random.default_rng(3)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (9, 7, 11, 5)]
    emb, pad = prefix(m, m.get_conditioning(cond_mel, None), texts)
    scalar = []
    for sp in ROWS4:
        eng.prefill(emb, pad, STEPS)
        scalar.append(eng.decode(STEPS, dict(sp, seed=SEED)).clone())
    assert all(c.shape == (4, STEPS) for c in scalar)
    for i, j in ((0, 1), (1, 2), (0, 2)):                  # the settings matter: no two of these runs agree on every row
        assert not torch.equal(scalar[i], scalar[j]), (i, j)
    rows = [dict(sp, seed=SEED, stream=b) for b, sp in enumerate(ROWS4)]
    eng._graphs.clear()
    got = {}
    for use_graph in (True, False):
        eng.prefill(emb, pad, STEPS)
        got[use_graph] = eng.decode(STEPS, rows, use_graph=use_graph).clone()
        for b in range(4):
            assert torch.equal(got[use_graph][b], scalar[b][b]), (use_graph, b, got[use_graph][b], scalar[b][b])
    assert len(eng._graphs) == 1
    # another assignment (the settings rotated over the rows): the same captured step, and every row still follows ITS settings
    perm = [2, 3, 0, 1]
    eng.prefill(emb, pad, STEPS)
    rot = eng.decode(STEPS, [dict(ROWS4[p], seed=SEED, stream=b) for b, p in enumerate(perm)])
    assert len(eng._graphs) == 1 and all(("per_row", True) in k[14] for k in eng._graphs)
    for b, p in enumerate(perm):
        assert torch.equal(rot[b], scalar[p][b]), (b, p)
    # dict-form sp keeps its own path and key
    eng.prefill(emb, pad, STEPS)
    assert torch.equal(eng.decode(STEPS, dict(ROWS4[1], seed=SEED)), scalar[1]) and len(eng._graphs) == 2
    with pytest.raises(ValueError):
        eng.decode(STEPS, rows[:3])
    with pytest.raises(ValueError):
        eng.decode(STEPS, rows[:3] + [dict(rows[3], top_k=0)])
    with pytest.raises(NotImplementedError):
        eng.decode_beam(STEPS, rows, 2)


def test_decode_refill_with_per_item_settings(model, cond_mel):
    """3 slots, 7 utterances, force_stop fixed per utterance (the refill schedule does not depend on the tokens).  Settings
    alternate {greedy, rep 10} {greedy, rep 1} {do_sample, k 1, T 0.7, rep 10} -- the last is argmax by construction.  Every
    utterance's codes equal the same queue run with scalar greedy parameters at that utterance's penalty."""
    m, eng = model, model.engine
    rng = np.random.default_rng(8)
    lens = [13, 11, 10, 8, 7, 6, 4]
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in lens]
    stops = [6, 11, 3, 9, 5, 12, 7]
    max_new, ce = 16, 4
    kinds = [dict(GREEDY, repetition_penalty=10.0), dict(GREEDY, repetition_penalty=1.0),
             dict(do_sample=True, temperature=0.7, top_k=1, top_p=1.0, repetition_penalty=10.0)]
    own = [dict(kinds[i % 3], seed=SEED + i, stream=0) for i in range(7)]
    conds = m.get_conditioning(cond_mel, None)

    def run(sp, with_settings, sp_default=None):
        queue = list(range(3, 7))
        emb, pad = prefix(m, conds, texts[:3])
        eng.prefill(emb, pad, 200)

        def feed(k):
            take = [queue.pop(0) for _ in range(min(k, len(queue)))]
            if not take:
                return []
            e, p = prefix(m, conds, [texts[i] for i in take])
            p = p.tolist()
            return [(e[j, p[j]:], stops[i]) + ((own[i],) if with_settings(i) else ()) for j, i in enumerate(take)]

        codes, leftover = eng.decode_refill(max_new, sp, feed, force_stop=stops[:3], check_every=ce, sp_default=sp_default)
        assert not leftover and len(codes) == 7 and eng.refill_stats["rows_refilled"] == 4
        return [c.cpu() for c in codes]

    scalar = {rep: run(dict(GREEDY, repetition_penalty=rep, seed=0), lambda i: False) for rep in (10.0, 1.0)}
    assert any(not torch.equal(a, b) for a, b in zip(scalar[10.0], scalar[1.0]))          # the penalty matters
    eng._graphs.clear()
    got = run(own[:3], lambda i: True)
    # utterance 5 brings no settings of its own: it gets the loop's default (its own, passed that way)
    got2 = run(own[:3], lambda i: i != 5, sp_default=own[5])
    assert len(eng._graphs) == 1
    for i in range(7):
        want = scalar[own[i]["repetition_penalty"]][i]
        assert want.numel() == stops[i] + 1
        assert torch.equal(got[i], want), (i, got[i], want)
        assert torch.equal(got2[i], want), (i, got2[i], want)
    with pytest.raises(ValueError):                         # settings on an item of a loop that runs under one dict
        run(dict(GREEDY, repetition_penalty=10.0, seed=0), lambda i: True)
    with pytest.raises(ValueError):                         # an item without settings and no default
        run(own[:3], lambda i: False)


def test_infer_batch_with_sampling_and_adapters(cond_mel):
    """IndexTTS.infer_batch(sampling=[...]): waveforms whose codes are the engine's under the resolved settings; with an attached
    adapter bank and adapter_ids it runs (finite, non-empty waveforms); num_beams = 3 is refused; infer_queue takes the same list."""
    from indextts.gpt.model import row_sampling_params
    from indextts.infer import IndexTTS
    from test_lora_bank_gpu import make_bank
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    sd = weights.gpt_state_dict(2)
    tts = IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0",
                                precision_config={"gpt": "bf16", "vocoder": "fp16"})
    rng = np.random.default_rng(5)
    texts = [torch.from_numpy(rng.integers(2, 12000, size=n)).to(torch.int32) for n in (9, 6, 8, 7)]
    gen = dict(do_sample=True, num_beams=1, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0)
    sampling = [dict(do_sample=False), dict(temperature=0.7, seed=(1 << 34) + 1), {}, dict(top_k=1, repetition_penalty=1.0)]
    kw = dict(max_mel_tokens=STEPS, force_stop=[8] * 4, return_codes=True, seed=77)
    wavs, codes = tts.infer_batch(cond_mel, texts, sampling=sampling, **kw, **gen)
    assert all(w.numel() == 8 * 1024 and torch.isfinite(w).all() for w in wavs)
    # the engine-level result under the resolved list
    g, eng = tts.gpt, tts.gpt.engine
    rows = row_sampling_params(sampling, 4, gen, 77)
    assert [r["stream"] for r in rows] == [0, 0, 2, 3] and rows[1]["seed"] == (1 << 34) + 1 and rows[2]["seed"] == 77
    conds, _ = tts._prompt_features(cond_mel)
    emb, pad = prefix(g, conds, texts)
    eng.prefill(emb, pad, STEPS, shared_rows=int(conds.shape[1]))
    want = eng.decode(STEPS, rows, force_stop=[8] * 4)
    want_np, lens = tts._squeeze_silence_host(want)
    for i in range(4):
        assert np.array_equal(codes[i].numpy(), want_np[i, : lens[i]]), i
    with pytest.raises(NotImplementedError):
        tts.infer_batch(cond_mel, texts, sampling=sampling, **kw, **dict(gen, num_beams=3))
    with pytest.raises(ValueError):
        tts.infer_batch(cond_mel, texts, sampling=sampling[:3], **kw, **gen)
    # the queue: 2 slots, the same four requests -- each keeps its own settings wherever it is placed
    q_wavs, q_codes = tts.infer_queue(cond_mel, texts, slots=2, max_mel_tokens=STEPS, force_stop=[8] * 4, seed=77, return_codes=True,
                                      check_every=4, sampling=sampling, **gen)
    assert len(q_wavs) == 4 and all(w.numel() > 0 and torch.isfinite(w).all() for w in q_wavs)
    # with voices: an adapter bank and per-row settings in one batch
    bank, _ = make_bank(sd, (8, 16), (2.0, 1.5))
    tts.gpt.attach_lora_bank(bank)
    v_wavs = tts.infer_batch(cond_mel, texts, adapter_ids=[0, 1, -1, 1], sampling=sampling, **dict(kw, return_codes=False), **gen)
    assert len(v_wavs) == 4 and all(w.numel() > 0 and torch.isfinite(w).all() for w in v_wavs)
    tts.gpt.detach_lora_bank()
