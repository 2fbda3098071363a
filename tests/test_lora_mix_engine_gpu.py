"""Per-row adapter BLENDS through the engine and the public interface (adapter_mix=...): a row speaks with a weighted mix of up to
four voices of the attached bank,  y = x W + sum_j w_j s_j (x A_j^T) B_j^T = [x | u] [W ; B_bank^T].

Every mix is held to a one-row run of the model whose checkpoint has that mix MERGED (W + sum_j w_j s_j A_j^T B_j^T, formed in fp32),
with the bounds test_lora_bank_gpu.py holds single voices to; mixes that name one adapter at weight 1 to the bits of the adapter_ids
path.  2 layers, 4 rows, one short text."""
import os

import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
MIXES = [{0: 1.0}, {0: 0.5, 2: 0.5}, None, {1: 0.25}]
IDS = [0, 2, -1, 0]
STEPS = 10


def make_factors(sd, ranks, scalings, layers=2, seed=3):
    """[(adapters, scaling)] on all four targets of every layer: the bank in the attach_lora_bank format."""
    g = torch.Generator().manual_seed(seed)
    bank = []
    for r, sc in zip(ranks, scalings):
        ad = {}
        for i in range(layers):
            for name in TARGETS:
                key = f"gpt.h.{i}.{name}"
                k_in, n_out = sd[key + ".weight"].shape
                ad[key] = (torch.randn(r, k_in, generator=g) * 0.02, torch.randn(n_out, r, generator=g) * 0.02)
        bank.append((ad, sc))
    return bank


def merged_state(sd, bank, mix):
    """The checkpoint with the mix merged: W + sum_j w_j s_j A_j^T B_j^T in fp32 (mix: {id: weight} or None)."""
    ms = dict(sd)
    for a, w in (mix or {}).items():
        ad, sc = bank[a]
        for key, (A, Bm) in ad.items():
            ms[key + ".weight"] = ms[key + ".weight"].float() + (A.t() @ Bm.t()) * (sc * w)
    return ms


def make_model(state, dtype):
    from indextts.gpt.model import UnifiedVoice
    cfg = dict(weights.reference_config()["gpt"], layers=2)
    m = UnifiedVoice(**cfg)
    m.load_state_dict(state)
    m.to(DEV).to(dtype).post_init_gpt2_config(kv_cache=True)
    return m


def key_of(mix):
    return tuple(sorted((mix or {}).items()))


class Blends:
    """Three adapters (ranks 4 / 8 / 16, different scalings), one text, and -- computed once, shared, never changed -- the one-row
    runs of the merged model of every mix the tests name."""
    KW = dict(do_sample=False, num_beams=1, repetition_penalty=10.0, max_generate_length=STEPS, return_logits=True)

    def __init__(self):
        self.sd = weights.gpt_state_dict(2)
        self.bank = make_factors(self.sd, (4, 8, 16), (2.0, 1.0, 0.5))
        g = np.load(os.path.join(G, "gpt_small.npz"))
        n0 = int(g["text_lens"][0])
        self.text1 = torch.from_numpy(g["text"][0:1, :n0]).to(DEV)
        self.text4 = self.text1.repeat(4, 1)
        self.cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
        self._single = {}
        self._bank_model = {}

    def merged_model(self, mix, dtype):
        return make_model(merged_state(self.sd, self.bank, mix), dtype)

    def single(self, mix, dtype):
        """(codes [1, n], logits [n, 1, V], latent [1, n, D] under the codes of MIXES[0]) of the mix's merged model run alone."""
        k = (key_of(mix), dtype)
        if k not in self._single:
            m = self.merged_model(mix, dtype)
            codes, logits = m.inference_speech(self.cond_mel, self.text1, **self.KW)
            c0 = codes if key_of(mix) == key_of(MIXES[0]) else self.single(MIXES[0], dtype)[0]
            self._single[k] = (codes.clone(), logits.clone(), self.latent(m, 1, c0).clone())
        return self._single[k]

    def latent(self, m, B, codes, **kw):
        n = self.text1.shape[1]
        return m(self.cond_mel, self.text1.repeat(B, 1), torch.tensor([n] * B), codes.repeat(B, 1) if codes.shape[0] == 1 else codes,
                 torch.tensor([codes.shape[1] * 1024] * B), return_latent=True, **kw)

    def fresh(self, dtype):
        return make_model(self.sd, dtype).attach_lora_bank(self.bank)

    def bank_model(self, dtype):
        if dtype not in self._bank_model:
            self._bank_model[dtype] = self.fresh(dtype)
        return self._bank_model[dtype]


@pytest.fixture(scope="module")
def blends():
    return Blends()


def test_every_row_speaks_with_its_own_mix_fp32(blends):
    """Prefill logits and 10 greedy-step logits of every row against that row's merged model decoded alone: < 1e-3 with equal codes
    (the bank's bound for this comparison); the latent pass with the same mixes < 1e-3.  The blended row differs from both of its
    ingredients by > 1e-2: the mix matters."""
    m = blends.bank_model(torch.float32)
    eng = m.engine
    assert eng.bank.n == 3 and eng.bank.rp == 16 and eng.bank.Kx == 64 and not eng._fold_now(4)
    codes, logits = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES, **blends.KW)
    assert eng._mix_host == [((0, 1.0),), ((0, 0.5), (2, 0.5)), (), ((1, 0.25),)] and eng._ids_host is None
    assert eng.adapter_mix.dtype == torch.uint8 and tuple(eng.adapter_mix.shape) == (eng._cap_b, 32)
    assert logits.shape[0] >= STEPS
    for row, mix in enumerate(MIXES):
        c, l, _ = blends.single(mix, torch.float32)
        err = (logits[:, row] - l[:, 0]).abs().max().item()
        print(f"row {row} mix {mix}: max |logit diff| {err:.3e}")
        assert err < 1e-3, (row, mix, err)
        assert torch.equal(codes[row], c[0]), (row, mix)
    assert (logits[:, 1] - logits[:, 0]).abs().max().item() > 1e-2
    assert (logits[:, 1] - blends.single({2: 1.0}, torch.float32)[1][:, 0]).abs().max().item() > 1e-2
    assert (logits[:, 1] - logits[:, 2]).abs().max().item() > 1e-2
    c0 = blends.single(MIXES[0], torch.float32)[0]
    lat = blends.latent(m, 4, c0, adapter_mix=MIXES)
    for row, mix in enumerate(MIXES):
        ref = blends.single(mix, torch.float32)[2]
        err = (lat[row] - ref[0]).abs().max().item()
        print(f"latent row {row} mix {mix}: max diff {err:.3e}")
        assert err < 1e-3, (row, mix, err)
    assert (lat[0] - lat[1]).abs().max().item() > 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_weight_one_mixes_are_the_id_path_bit_for_bit(blends, dtype):
    """adapter_mix=[0, 2, -1, 0] against adapter_ids=[0, 2, -1, 0]: torch.equal logits and codes (the mix launch accumulates in the
    id launch's order and multiplies by exactly 1).  A {0: 0.0} row: the base row's codes and logits, bit for bit."""
    m = blends.bank_model(dtype)
    ci, li = m.inference_speech(blends.cond_mel, blends.text4, adapter_ids=IDS, **blends.KW)
    ci, li = ci.clone(), li.clone()
    cm, lm = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=IDS, **blends.KW)
    assert torch.equal(cm, ci) and torch.equal(lm, li)
    cd, ld = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=[{0: 1.0}, [(2, 1.0)], {}, 0], **blends.KW)
    assert torch.equal(cd, ci) and torch.equal(ld, li)
    cz, lz = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=[{0: 0.0}, None, {0: 0.0, 1: 0.0}, 0], **blends.KW)
    assert torch.equal(cz[0], cz[1]) and torch.equal(lz[:, 0], lz[:, 1]) and torch.equal(lz[:, 2], lz[:, 1])
    assert torch.equal(lz[:, 1], li[:, 2]) and torch.equal(lz[:, 3], li[:, 0])
    assert (li[:, 0] - li[:, 2]).abs().max().item() > 1e-2


def test_mix_bf16_tracks_the_merged_models_and_graph_equals_eager(blends):
    """bf16, teacher-forced with each row's own greedy codes (those of its merged bf16 model): logits RMS < 4e-2 against the merged
    bf16 model of each mix -- the bank's bound; the two sides differ in the same two places of rounding (W + sum w s A^T B^T rounded
    once, against W, s A, B and u rounded each).  The single-voice rows (0, 2 = base, 3 = one voice at 0.25) are measured beside
    the blended row 1 in the same run and all figures are printed (profiles/lora_mix_parity.txt).  Free-running, the
    graph-replayed loop reproduces the eager loop token for token."""
    m = blends.bank_model(torch.bfloat16)
    eng = m.engine
    refs = [blends.single(mix, torch.bfloat16) for mix in MIXES]
    steps = min(r[0].shape[1] for r in refs)
    force = torch.cat([r[0][:, :steps] for r in refs], 0).to(torch.int32).to(DEV)            # [4, n]
    conds = m.get_conditioning(blends.cond_mel, None)
    emb, pad = m.prefix_rows(conds, blends.text4)
    sp = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=1.0, seed=0)
    out = [eng.prefill(emb, pad, steps + 2, adapter_mix=MIXES)[:4].clone()]
    eng.force_stop[:4] = -1
    skip, eng.skip_finished = eng.skip_finished, False
    try:
        for s in range(1, steps):
            eng._sample(4, sp)
            eng.tokens[:4] = force[:, s - 1]
            eng.history[:4, s - 1] = force[:, s - 1]
            eng.finished[:4] = 0
            eng._step_transformer(4)
            out.append(eng.logits[:4].clone())
    finally:
        eng.skip_finished = skip
    got = torch.stack(out, 0)
    figures = []
    for row, (c, l, _) in enumerate(refs):
        d = got[:, row] - l[:steps, 0]
        rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
        figures.append(rms)
        print(f"bf16 row {row} mix {MIXES[row]}: rms {rms:.3e} max {mx:.3e}")
    print(f"bf16 blended row / worst single-voice row: {figures[1] / max(figures[0], figures[2], figures[3]):.3f}")
    for row, rms in enumerate(figures):
        assert rms < 4e-2, (row, rms)
    eng._graphs.clear()
    ca, la = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES, **blends.KW)
    assert len(eng._graphs) == 1 and all(k[-1][0] == "bank-mix" for k in eng._graphs)
    eng.prefill(emb, pad, STEPS, adapter_mix=MIXES)
    cb, lb = eng.decode(STEPS, dict(sp, repetition_penalty=10.0), use_graph=False, return_logits=True)
    assert torch.equal(ca, cb) and torch.equal(la, lb)


def test_mixes_are_data_not_structure(blends):
    """A second run on the same engine with the mixes permuted across the rows replays the same captured step (no new graph) and
    gives every mix the logits it had in its earlier row."""
    m = blends.bank_model(torch.float32)
    eng = m.engine
    c1, l1 = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES, **blends.KW)
    c1, l1 = c1.clone(), l1.clone()
    graphs = len(eng._graphs)
    assert graphs >= 1
    perm = [2, 0, 3, 1]
    c2, l2 = m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=[MIXES[p] for p in perm], **blends.KW)
    assert len(eng._graphs) == graphs
    for row, p in enumerate(perm):
        assert (l2[:, row] - l1[:, p]).abs().max().item() < 1e-3 and torch.equal(c2[row], c1[p]), (row, p)
    # the key says WHICH shrink launch the step holds and the bank's shape, never the records
    assert sorted({k[-1][0] for k in eng._graphs}) in (["bank-mix"], ["bank", "bank-mix"])
    assert all(k[-1][1:] == eng.bank.sig for k in eng._graphs)
    assert not any("0.5" in repr(k[-1]) or "0.25" in repr(k[-1]) for k in eng._graphs)


def test_nothing_leaks_between_the_mix_path_and_the_id_path(blends):
    """One engine alternates mix and id batches: after a mix batch an adapter_ids batch gives the bits of an engine that never saw a
    mix, after an id batch a mix batch gives the bits of an engine that never saw an id batch.  A fork keeps its own table."""
    run = lambda m, **kw: tuple(t.clone() for t in m.inference_speech(blends.cond_mel, blends.text4, **kw, **blends.KW))   # noqa: E731
    other = [{1: 1.0}, {1: -0.5, 2: 1.5}, {0: 0.3, 1: 0.3, 2: 0.4}, 2]
    only_ids = run(blends.fresh(torch.float32), adapter_ids=IDS)
    only_mix = run(blends.fresh(torch.float32), adapter_mix=other)
    m = blends.fresh(torch.float32)
    eng = m.engine
    tag = lambda: eng._graph_key("token", 4, dict(do_sample=False))[-1]   # noqa: E731  (the part of the key the bank adds)
    assert tag() == ("bank",) + eng.bank.sig
    run(m, adapter_mix=MIXES)
    assert tag() == ("bank-mix",) + eng.bank.sig
    got = run(m, adapter_ids=IDS)
    assert eng._mix_host is None and tag() == ("bank",) + eng.bank.sig
    assert torch.equal(got[0], only_ids[0]) and torch.equal(got[1], only_ids[1])
    got = run(m, adapter_mix=other)
    assert eng._ids_host is None
    assert torch.equal(got[0], only_mix[0]) and torch.equal(got[1], only_mix[1])
    got = run(m)                                         # no voices named: all base, on the id launch
    assert eng._mix_host is None and torch.equal(got[1][:, 0], only_ids[1][:, 2])
    # a fork: its own table, written by its own batches only
    run(m, adapter_mix=other)
    table = eng.adapter_mix.clone()
    fork = m.replica()
    f = run(fork, adapter_mix=MIXES)
    assert fork.engine.adapter_mix.data_ptr() != eng.adapter_mix.data_ptr() and torch.equal(eng.adapter_mix, table)
    assert fork.engine._mix_host != eng._mix_host
    assert not torch.equal(f[1], only_mix[1])
    got = run(m, adapter_mix=other)                      # the parent is where it was
    assert torch.equal(got[1], only_mix[1])
    m.detach_lora_bank()                                 # detaching clears the table with the ids
    assert eng._mix_host is None and (eng.adapter_mix.view(torch.int32)[:, 0::2] == -1).all()


def test_refusals(blends):
    m = blends.bank_model(torch.float32)
    eng = m.engine
    kw = dict(blends.KW, max_generate_length=2)
    with pytest.raises(NotImplementedError):              # beams with a mix
        m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES, **dict(kw, num_beams=3, return_logits=False))
    conds = m.get_conditioning(blends.cond_mel, None)
    emb, pad = m.prefix_rows(conds, blends.text4)
    with pytest.raises(NotImplementedError):
        eng.prefill(emb, pad, 4, beams=3, adapter_mix=MIXES)
    with pytest.raises(NotImplementedError):
        eng.decode_refill(4, {}, lambda k: [])
    plain = make_model(blends.sd, torch.float32)
    with pytest.raises(ValueError):                       # a mix without a bank
        plain.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES, **kw)
    with pytest.raises(ValueError):
        blends.latent(plain, 4, blends.single(MIXES[0], torch.float32)[0], adapter_mix=MIXES)
    with pytest.raises(ValueError):                       # ids and mixes together
        m.inference_speech(blends.cond_mel, blends.text4, adapter_ids=IDS, adapter_mix=MIXES, **kw)
    with pytest.raises(ValueError):                       # wrong number of rows
        m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=MIXES[:3], **kw)
    with pytest.raises(ValueError):                       # id >= n
        m.inference_speech(blends.cond_mel, blends.text4, adapter_mix=[{3: 1.0}, None, None, None], **kw)
    # the cached prompt belongs to the mixes it was prefilled under
    eng.prefill(emb, pad, 4, adapter_mix=MIXES)
    mel = torch.zeros(8, eng.D, device=DEV)
    with pytest.raises(ValueError, match="other adapter mixes"):
        eng.latent_mel_rows(mel, [2] * 4, adapter_mix=[{0: 1.0}, {0: 0.5, 2: 0.25}, None, {1: 0.25}])
    with pytest.raises(ValueError):
        eng.latent_mel_rows(mel, [2] * 4, adapter_ids=IDS)
    eng.prefill(emb, pad, 4, adapter_ids=IDS)
    with pytest.raises(ValueError, match="other adapter mixes"):
        eng.latent_mel_rows(mel, [2] * 4, adapter_mix=IDS)
    torch.cuda.synchronize()


def test_infer_batch_blends_two_voices_across_four_rows():
    """IndexTTS.infer_batch(adapter_mix=...) end to end (token loop, latent pass over the cached prompt, vocoder), greedy with
    force_stop: the two rows of the 50 / 50 blend give identical codes and waveforms, which differ from either voice alone; every
    waveform is finite and of the forced length.  Composes with per-row sampling settings and a prompt per row; infer_queue and
    infer (the REST service's call) keep refusing a bank."""
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    sd = weights.gpt_state_dict(2)
    tts = IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0",
                                precision_config={"gpt": "bf16", "vocoder": "fp16"})
    bank = make_factors(sd, (8, 16), (2.0, 1.5))
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    text = torch.from_numpy(np.random.default_rng(5).integers(2, 12000, size=9)).to(torch.int32)
    gen = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
    kw = dict(max_mel_tokens=12, force_stop=[8] * 4, return_codes=True)
    half = {0: .5, 1: .5}
    mix = [half, 0, half, 1]
    with pytest.raises(ValueError):
        tts.infer_batch(cond_mel, [text] * 4, adapter_mix=mix, **kw, **gen)                  # no bank yet
    tts.gpt.attach_lora_bank(bank)
    wavs, codes = tts.infer_batch(cond_mel, [text] * 4, adapter_mix=mix, **kw, **gen)
    assert all(w.numel() == 8 * 1024 and torch.isfinite(w).all() for w in wavs)
    assert torch.equal(codes[0], codes[2]) and torch.equal(wavs[0], wavs[2])
    assert not torch.equal(wavs[0], wavs[1]) and not torch.equal(wavs[0], wavs[3]) and not torch.equal(wavs[1], wavs[3])
    by_id = tts.infer_batch(cond_mel, [text] * 4, adapter_ids=[0, 0, 1, 1], **kw, **gen)[0]
    assert torch.equal(by_id[0], wavs[1]) and torch.equal(by_id[2], wavs[3])                 # an int in a mix IS that voice
    with pytest.raises(ValueError):
        tts.infer_batch(cond_mel, [text] * 4, adapter_ids=[0, 0, 1, 1], adapter_mix=mix, **kw, **gen)
    with pytest.raises(NotImplementedError):
        tts.infer_batch(cond_mel, [text] * 4, adapter_mix=mix, max_mel_tokens=12, **dict(gen, num_beams=3))
    # beside per-row sampling settings and a prompt per row (both per row already)
    cond2 = torch.from_numpy(synth.uniform("in.cond_mel2", (1, 100, 90), -6.0, 2.0)).to(DEV)
    rows = [dict(do_sample=False)] * 4
    w2, c2 = tts.infer_batch([cond_mel, cond2, cond_mel, cond2], [text] * 4, adapter_mix=mix, sampling=rows, **kw, **gen)
    assert all(w.numel() == 8 * 1024 and torch.isfinite(w).all() for w in w2)
    assert torch.equal(c2[0], c2[2]) and torch.equal(w2[0], w2[2])
    assert not torch.equal(w2[1], wavs[1])                                                   # row 1: the other prompt
    with pytest.raises(NotImplementedError):
        tts.infer_queue(cond_mel, [text] * 4, slots=2, max_mel_tokens=12, **gen)
    with pytest.raises(NotImplementedError):
        tts._generate(None, text[None].to(DEV), dict(gen), 12)
    tts.gpt.detach_lora_bank()
