"""Per-row LoRA adapter bank (GPTEngine.attach_lora_bank + itts_lora_shrink): many fine-tuned voices in one batch.

The identity under test:  y = x W + s_a (x A_a^T) B_a^T = [x | u] [W ; B_bank^T]  with a = the row's adapter id.  The kernel is held
to an fp64 reference on its rounded operands; the engine to one-row runs of models whose checkpoint has the row's adapter merged
(the construction and the bounds of test_engines_gpu.py::test_runtime_lora_equals_merged_checkpoint)."""
import os

import numpy as np
import pytest
import torch

import synth
import weights

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
RES = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
IDS = [0, 2, -1, 0]
STEPS = 10


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [64, 1280, 5120])
def test_shrink_kernel_against_fp64_on_the_rounded_operands(dtype, K):
    """n = 3 adapters of ranks 4 / 16 / 40 (rp = 48, Kx = 144 -> 160: the padding to 32 is exercised), M = 5 (a partial tile) and
    37 (three tiles, the last partial), both output forms, ids with -1 / a repeated id / all rows equal.  Own slot:
    |got - ref| <= RES[T] |ref| + 1e-5 sum_k |x a| (one rounding of the storage type + fp32 accumulation); foreign slots, padding
    columns and the padding rows of the packed tail exactly 0.  Every id set is written into the SAME buffer: nothing of the
    call before it may survive."""
    from indextts import _native as nat
    n, ranks, rp = 3, (4, 16, 40), 48
    Kx = nat.lora_kx(n, rp)
    assert Kx == 160
    g = torch.Generator().manual_seed(K)
    A32 = torch.zeros(n, rp, K)
    for a, r in enumerate(ranks):
        A32[a, :r] = torch.randn(r, K, generator=g) * 0.05 * (a + 1)       # (a + 1): the scaling, folded in at fp32
    A = A32.to(dtype).to(DEV).contiguous()
    Ad = A.double().cpu()
    for M in (5, 37):
        x = torch.randn(M, K, generator=g).to(dtype).to(DEV).contiguous()
        xd = x.double().cpu()
        Mp = nat.packed_rows(M)
        id_sets = [[(i * 7) % 4 - 1 for i in range(M)], [1] * M, [-1] + [2] * (M - 1)]
        assert -1 in id_sets[0] and len(set(id_sets[0])) == 4
        packed = torch.cat([nat.pack_activation(x), torch.full((Mp * Kx,), 7.0, dtype=dtype, device=DEV)])
        rows = torch.full((M, K + Kx), 7.0, dtype=dtype, device=DEV)
        rows[:, :K] = x
        for ids in id_sets:
            ids_t = torch.tensor(ids, dtype=torch.int32, device=DEV)
            nat.lora_shrink(packed, ids_t, A, packed[Mp * K:], M, K, x_packed=True, u_packed=True)
            nat.lora_shrink(x, ids_t, A, rows[:, K:], M, K, ldu=K + Kx)
            whole = nat.unpack_activation(packed, Mp, K + Kx)
            assert torch.equal(whole[:M, :K], x) and torch.equal(rows[:, :K], x)          # the operand's front is not touched
            assert (whole[M:, K:] == 0).all()                                               # padding rows of the tail
            for form, u in (("packed", whole[:M, K:]), ("rows", rows[:, K:])):
                u = u.double().cpu()
                for m, a in enumerate(ids):
                    own = slice(a * rp, (a + 1) * rp) if a >= 0 else slice(0, 0)
                    mask = torch.ones(Kx, dtype=torch.bool)
                    mask[own] = False
                    assert (u[m][mask] == 0).all(), (form, M, m, a)
                    if a >= 0:
                        ref = Ad[a] @ xd[m]
                        mag = Ad[a].abs() @ xd[m].abs()
                        err = (u[m][own] - ref).abs()
                        assert (err <= RES[dtype] * ref.abs() + 1e-5 * mag).all(), (form, M, m, a, err.max().item())
                        assert (u[m][own][ranks[a]:] == 0).all()
            assert torch.equal(whole[:M, K:], rows[:, K:])                                  # the two forms: same bits


def test_shrink_refuses_shapes_outside_its_limits():
    from indextts import _native as nat
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(4, dtype=torch.int32, device=DEV)
    u = torch.zeros(4, 512 + 64, dtype=torch.bfloat16, device=DEV)
    for n, rp in ((1, 80), (9, 64), (1, 24)):              # rank > 64; Kx > 512; rp not a multiple of 16
        with pytest.raises(nat.NativeError):
            nat.lora_shrink(x, ids, torch.zeros(n, rp, 64, dtype=torch.bfloat16, device=DEV), u, 4, 64, ldu=u.shape[1])
    with pytest.raises(nat.NativeError):                   # K % KS != 0
        nat.lora_shrink(x[:, :48].contiguous(), ids, torch.zeros(1, 16, 48, dtype=torch.bfloat16, device=DEV), u, 4, 48, ldu=u.shape[1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- engine
def make_bank(sd, ranks, scalings, layers=2, seed=3):
    """[(adapters, scaling)] on all four targets of every layer, and the merged checkpoint of every voice."""
    g = torch.Generator().manual_seed(seed)
    bank, merged = [], []
    for r, sc in zip(ranks, scalings):
        ad, ms = {}, dict(sd)
        for i in range(layers):
            for name in TARGETS:
                key = f"gpt.h.{i}.{name}"
                k_in, n_out = sd[key + ".weight"].shape
                A = torch.randn(r, k_in, generator=g) * 0.02
                Bm = torch.randn(n_out, r, generator=g) * 0.02
                ad[key] = (A, Bm)
                ms[key + ".weight"] = sd[key + ".weight"] + (A.t() @ Bm.t()) * sc
        bank.append((ad, sc))
        merged.append(ms)
    return bank, merged


def make_model(state, dtype):
    from indextts.gpt.model import UnifiedVoice
    cfg = dict(weights.reference_config()["gpt"], layers=2)
    m = UnifiedVoice(**cfg)
    m.load_state_dict(state)
    m.to(DEV).to(dtype).post_init_gpt2_config(kv_cache=True)
    return m


class Voices:
    """Three adapters (ranks 4 / 8 / 16, different scalings), one text, and -- computed once, shared, never changed -- the one-row
    runs of the merged single-voice models (voice -1 = the base checkpoint)."""
    KW = dict(do_sample=False, num_beams=1, repetition_penalty=10.0, max_generate_length=STEPS, return_logits=True)

    def __init__(self):
        self.sd = weights.gpt_state_dict(2)
        self.bank, self.merged = make_bank(self.sd, (4, 8, 16), (2.0, 1.0, 0.5))
        g = np.load(os.path.join(G, "gpt_small.npz"))
        n0 = int(g["text_lens"][0])
        self.text1 = torch.from_numpy(g["text"][0:1, :n0]).to(DEV)
        self.text4 = self.text1.repeat(4, 1)
        self.cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
        self._single = {}
        self._bank_model = {}

    def state(self, v):
        return self.sd if v < 0 else self.merged[v]

    def single(self, v, dtype):
        """(codes [1, n], logits [n, 1, V], latent [1, n, D]) of the merged model of voice v run alone."""
        if (v, dtype) not in self._single:
            m = make_model(self.state(v), dtype)
            codes, logits = m.inference_speech(self.cond_mel, self.text1, **self.KW)
            self._single[(v, dtype)] = (codes.clone(), logits.clone(), self.latent(m, 1, codes).clone())
        return self._single[(v, dtype)]

    def latent(self, m, B, codes, **kw):
        n = self.text1.shape[1]
        return m(self.cond_mel, self.text1.repeat(B, 1), torch.tensor([n] * B), codes.repeat(B, 1) if codes.shape[0] == 1 else codes,
                 torch.tensor([codes.shape[1] * 1024] * B), return_latent=True, **kw)

    def bank_model(self, dtype):
        if dtype not in self._bank_model:
            self._bank_model[dtype] = make_model(self.sd, dtype).attach_lora_bank(self.bank)
        return self._bank_model[dtype]


@pytest.fixture(scope="module")
def voices():
    return Voices()


def test_every_row_speaks_with_its_own_adapter_fp32(voices):
    """Four rows of one text, ids [0, 2, -1, 0]: prefill logits and 10 greedy-step logits of every row agree (< 1e-3, equal codes)
    with a one-row run of the model whose checkpoint has THAT adapter merged; row 2 with the base model; rows 0 and 1 differ by
    > 1e-2 (the adapters matter and are not mixed up)."""
    m = voices.bank_model(torch.float32)
    eng = m.engine
    assert eng.bank.n == 3 and eng.bank.rp == 16 and eng.bank.Kx == 64 and not eng._fold_now(4)
    codes, logits = m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **voices.KW)
    assert eng.adapter_ids[:4].tolist() == IDS
    for row, v in enumerate(IDS):
        c, l, _ = voices.single(v, torch.float32)
        err = (logits[:, row] - l[:, 0]).abs().max().item()
        print(f"row {row} voice {v}: max |logit diff| {err:.3e}")
        assert err < 1e-3, (row, v, err)
        assert torch.equal(codes[row], c[0]), (row, v)
    assert (logits[:, 0] - logits[:, 1]).abs().max().item() > 1e-2
    assert (logits[:, 0] - logits[:, 2]).abs().max().item() > 1e-2


def test_latent_pass_per_row_adapters_fp32(voices):
    """forward(return_latent=True, adapter_ids=...) over the same four rows against each voice's merged model (< 1e-3)."""
    m = voices.bank_model(torch.float32)
    codes = voices.single(0, torch.float32)[0]
    lat = voices.latent(m, 4, codes, adapter_ids=IDS)
    for row, v in enumerate(IDS):
        ref = voices.latent(make_model(voices.state(v), torch.float32), 1, codes) if v != 0 else voices.single(0, torch.float32)[2]
        err = (lat[row] - ref[0]).abs().max().item()
        print(f"latent row {row} voice {v}: max diff {err:.3e}")
        assert err < 1e-3, (row, v, err)
    assert (lat[0] - lat[1]).abs().max().item() > 1e-3


def test_bank_bf16_tracks_the_merged_models_and_graph_equals_eager(voices):
    """bf16, rows and ids as above, teacher-forced with each voice's own greedy codes: the logits stay within the bf16 bound of
    the merged single-voice bf16 models (RMS < 4e-2; the two differ in where values are rounded: W + s A^T B^T rounded once against
    W, s A, B and u rounded each).  Free-running, the graph-replayed loop reproduces the eager loop token for token."""
    m = voices.bank_model(torch.bfloat16)
    eng = m.engine
    refs = [voices.single(v, torch.bfloat16) for v in IDS]
    force = torch.cat([r[0] for r in refs], 0).to(torch.int32).to(DEV)            # [4, n]
    steps = force.shape[1]
    conds = m.get_conditioning(voices.cond_mel, None)
    emb, pad = m.prefix_rows(conds, voices.text4)
    sp = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=1.0, seed=0)
    out = [eng.prefill(emb, pad, steps + 2, adapter_ids=IDS)[:4].clone()]
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
    for row, (c, l, _) in enumerate(refs):
        d = got[:, row] - l[:steps, 0]
        rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
        print(f"bf16 row {row} voice {IDS[row]}: rms {rms:.3e} max {mx:.3e}")
        assert rms < 4e-2, (row, rms, mx)
    eng._graphs.clear()
    ca, la = m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **voices.KW)
    assert len(eng._graphs) == 1
    eng.prefill(emb, pad, STEPS, adapter_ids=IDS)
    sp10 = dict(sp, repetition_penalty=10.0)
    cb, lb = eng.decode(STEPS, sp10, use_graph=False, return_logits=True)
    assert torch.equal(ca, cb) and torch.equal(la, lb)


def test_ids_are_data_not_structure(voices):
    """A second run on the same engine with the ids permuted replays the same captured step (no new graph) and every row's
    logits follow its voice."""
    m = voices.bank_model(torch.float32)
    eng = m.engine
    _, l1 = m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **voices.KW)
    graphs = len(eng._graphs)
    assert graphs >= 1
    perm = [2, 0, 0, -1]
    c2, l2 = m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=perm, **voices.KW)
    assert len(eng._graphs) == graphs
    for row, v in enumerate(perm):
        c, l, _ = voices.single(v, torch.float32)
        assert (l2[:, row] - l[:, 0]).abs().max().item() < 1e-3 and torch.equal(c2[row], c[0]), (row, v)
        assert (l2[:, row] - l1[:, IDS.index(v)]).abs().max().item() < 1e-3       # the run in which that voice sat in row IDS.index(v)
    assert all(k[-1] == ("bank",) + eng.bank.sig for k in eng._graphs)             # the key carries the bank's shape, never the ids


def test_nothing_leaks_into_the_base_path(voices):
    """An engine that had a bank attached and detached gives the bits of one that never had one; a fork taken before the attach
    is unaffected; the bank itself follows the fork rule of attach_lora."""
    never = make_model(voices.sd, torch.float32)
    key_new = never.engine._graph_key("token", 4, dict(do_sample=False))
    want = never.inference_speech(voices.cond_mel, voices.text4, **voices.KW)[1]
    key_run = never.engine._graph_key("token", 4, dict(do_sample=False))
    m = make_model(voices.sd, torch.float32)
    fork = m.replica()
    m.attach_lora_bank(voices.bank)
    assert m.engine.bank is not None and fork.engine.bank is None and "bank_w_o" not in fork.engine.layers[0]
    assert m.engine._graph_key("token", 4, dict(do_sample=False))[:-1] == key_new              # the key only GAINS the bank's signature
    got = m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **voices.KW)[1]
    assert (got - want).abs().max().item() > 1e-2
    assert torch.equal(fork.inference_speech(voices.cond_mel, voices.text4, **voices.KW)[1], want)
    fork2 = m.replica()                                  # forked WITH the bank: keeps it when the parent detaches
    m.detach_lora_bank()
    assert m.engine.bank is None and not any(k.startswith("bank_") for k in m.engine.layers[0])
    assert torch.equal(m.inference_speech(voices.cond_mel, voices.text4, **voices.KW)[1], want)
    assert m.engine._graph_key("token", 4, dict(do_sample=False)) == key_run
    assert torch.equal(fork2.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **voices.KW)[1], got)
    # a target no adapter names keeps its base weight and gets no extended copy
    only = [({k: v for k, v in ad.items() if k.endswith("attn.c_proj")}, sc) for ad, sc in voices.bank]
    m.attach_lora_bank(only)
    assert "bank_w_o" in m.engine.layers[0] and "bank_w_qkv" not in m.engine.layers[0] and "bank_a_w_pr" not in m.engine.layers[1]
    m.detach_lora_bank()


def test_refusals(voices, monkeypatch):
    m = voices.bank_model(torch.float32)
    single = voices.bank[0]
    with pytest.raises(ValueError):                       # bank and attach_lora together, either order
        m.attach_lora(*single)
    plain = make_model(voices.sd, torch.float32)
    plain.attach_lora(*single)
    with pytest.raises(ValueError):
        plain.attach_lora_bank(voices.bank)
    plain.attach_lora(None)
    kw = dict(voices.KW, max_generate_length=2)
    with pytest.raises(ValueError):                       # ids without a bank
        plain.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **kw)
    with pytest.raises(ValueError):                       # id >= n
        m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=[0, 3, 0, 0], **kw)
    with pytest.raises(ValueError):                       # id < -1
        m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=[0, -2, 0, 0], **kw)
    with pytest.raises(ValueError):                       # wrong length
        m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=[0, 1, 2], **kw)
    with pytest.raises(ValueError):
        voices.latent(m, 4, voices.single(0, torch.float32)[0], adapter_ids=[0, 1])
    with pytest.raises(NotImplementedError):              # beams with ids
        m.inference_speech(voices.cond_mel, voices.text4, adapter_ids=IDS, **dict(kw, num_beams=3, return_logits=False))
    with pytest.raises(NotImplementedError):
        m.engine.decode_refill(4, {}, lambda k: [])
    monkeypatch.setenv("ITTS_PACKED_ACT", "0")
    rowmajor = make_model(voices.sd, torch.float32)
    with pytest.raises(ValueError):
        rowmajor.attach_lora_bank(voices.bank)


def test_infer_batch_two_voices_across_four_rows():
    """IndexTTS.infer_batch(adapter_ids=...) end to end (token loop, latent pass over the cached prompt, vocoder): rows of the
    same voice with the same text and seed give identical waveforms, rows of different voices do not; infer_queue and
    infer (the REST service's call) refuse a bank."""
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    sd = weights.gpt_state_dict(2)
    tts = IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0",
                                precision_config={"gpt": "bf16", "vocoder": "fp16"})
    bank, _ = make_bank(sd, (8, 16), (2.0, 1.5))
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    text = torch.from_numpy(np.random.default_rng(5).integers(2, 12000, size=9)).to(torch.int32)
    gen = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
    kw = dict(max_mel_tokens=12, force_stop=[8] * 4, return_codes=True)
    with pytest.raises(ValueError):
        tts.infer_batch(cond_mel, [text] * 4, adapter_ids=[0, 1, 0, 1], **kw, **gen)        # no bank yet
    tts.gpt.attach_lora_bank(bank)
    wavs, codes = tts.infer_batch(cond_mel, [text] * 4, adapter_ids=[0, 1, 0, 1], **kw, **gen)
    assert all(w.numel() == 8 * 1024 and torch.isfinite(w).all() for w in wavs)
    assert torch.equal(codes[0], codes[2]) and torch.equal(codes[1], codes[3])
    assert torch.equal(wavs[0], wavs[2]) and torch.equal(wavs[1], wavs[3])
    assert not torch.equal(wavs[0], wavs[1])
    with pytest.raises(NotImplementedError):
        tts.infer_queue(cond_mel, [text] * 4, slots=2, max_mel_tokens=12, **gen)
    with pytest.raises(NotImplementedError):
        tts._generate(None, text[None].to(DEV), dict(gen), 12)
    tts.gpt.detach_lora_bank()
    base = tts.infer_batch(cond_mel, [text] * 4, **kw, **gen)[0]
    assert not torch.equal(base[0], wavs[0])
