"""The FP8 KV cache engine (GPTEngine(kv_dtype="fp8")) end to end on the small synthetic GPT (2 layers, full width, 4 rows): exact
properties (graph / eager, one captured step for every scale table, slot refill against the static batch, pool size, export_kv,
FP8 weights underneath), the refusals, calibration, and accuracy against oracle/gpt_ref.py (fp64 / fp32, unquantised K / V).

Accuracy rule.  Teacher-forced logits over the prefill and 12 decode steps, the oracle's greedy tokens forced, against the oracle on
the same weights; the 16-bit-cache engine's error against the same oracle is measured beside it.  The FP8-cache error must stay
within FACTOR x the 16-bit engine's error (max-abs and RMS).  Measured on an MI355X (profiles/kv8_engine_parity.txt):
    max-abs  fp8 cache 1.549e-01   16-bit cache 3.022e-02   ratio 5.12
    rms      fp8 cache 2.785e-02   16-bit cache 6.508e-03   ratio 4.28        (logits of RMS ~1)
    top-1 agreement with the oracle over all 52 (step, row) pairs: fp8 cache 0.904, 16-bit cache 0.942
(calibrated scales and scales of 1.0 give the same figures to three digits: E4M3 is a floating-point grid, a power-of-two scale
moves only its range).  FACTOR = 6.5: the measured 5.12 with a quarter on top, the margin test_w8_engine_gpu.py uses.
FACTOR covers the measured ratio with a margin for code flips at rounding boundaries between machines; the reference is the oracle,
never the engine under test.  Top-1 agreement is asserted on the (step, row) pairs whose oracle top-2 margin exceeds twice the
measured max-abs error (MAXABS)."""
import numpy as np
import pytest
import torch

import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS, D, HEADS, STEPS, B = 2, 1280, 20, 12, 4
FACTOR = 6.5          # err_fp8 <= FACTOR x err_16 (see the module docstring)
MAXABS = 0.16         # measured max-abs logit error of the FP8-cache engine (1.549e-01), rounded up
GREEDY = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=10.0, seed=0)
LENS = (11, 4, 8, 6)


@pytest.fixture(scope="module")
def world():
    """Weights, prompt, the oracle's teacher-forced trace and the engines: computed once, shared, left unchanged."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts.gpt.engine import GPTEngine
    from oracle import gpt_ref
    W = {k: v.float() for k, v in weights.gpt_state_dict(LAYERS, with_conditioner=False).items()}
    g = torch.Generator().manual_seed(3)
    conds = torch.randn(1, 32, D, generator=g) * 0.5
    rng = np.random.default_rng(7)
    text = torch.ones(B, max(LENS), dtype=torch.int64)               # unequal lengths: right-padded with the stop token (1)
    for b, n in enumerate(LENS):
        text[b, :n] = torch.from_numpy(rng.integers(2, 12000, size=n))
    emb, mask, pad = gpt_ref.prepare_gpt_inputs(conds, text, W)
    lg, past = gpt_ref.decode_prefill(emb, mask, W)
    ref_logits, toks = [lg], []
    for s in range(1, STEPS + 1):
        tok = lg.argmax(-1)
        toks.append(tok)
        mask = torch.cat([mask, torch.ones(B, 1, dtype=torch.bool)], 1)
        lg, past = gpt_ref.decode_step(tok, s, mask, past, W)
        ref_logits.append(lg)
    mk = lambda **kw: GPTEngine(W, LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, **kw)  # noqa: E731
    return dict(W=W, emb=emb, pad=pad.to(torch.int32), ref_logits=ref_logits, toks=toks, kv8=mk(kv_dtype="fp8"), bf16=mk(),
                w8kv8=mk(kv_dtype="fp8", weight_dtype="fp8"))


def pow2_table(seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(LAYERS, 2, HEADS), torch.randint(lo, hi + 1, (LAYERS, 2, HEADS), generator=g))


def teacher_forced(eng, w):
    """(max-abs, rms, top-1 agreement on decisive rows, decisive rows) of the logits over the prefill and STEPS decode steps."""
    lg = eng.prefill(w["emb"], w["pad"], STEPS + 2)
    got = [lg.float().cpu().clone()]
    for s in range(1, STEPS + 1):
        eng._sample(B, GREEDY)
        eng.tokens[:B] = w["toks"][s - 1].to(torch.int32).to(DEV)
        eng.history[:B, s - 1] = eng.tokens[:B]
        eng._step_transformer(B)
        got.append(eng.logits[:B].float().cpu().clone())
    got, ref = torch.stack(got).double(), torch.stack(w["ref_logits"]).double()
    err = (got - ref).abs()
    top2 = ref.topk(2, -1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2 * MAXABS
    agree = (got.argmax(-1) == ref.argmax(-1))
    return err.max().item(), err.pow(2).mean().sqrt().item(), bool(agree[decisive].all()), int(decisive.sum()), float(agree.double().mean())


def test_accuracy_against_the_oracle_beside_the_16_bit_cache(world):
    e8 = world["kv8"]
    e8.calibrate_kv_scales(world["emb"], world["pad"])
    m8, r8, a8, n8, t8 = teacher_forced(e8, world)
    m16, r16, a16, n16, t16 = teacher_forced(world["bf16"], world)
    print(f"kv8 parity | logits max-abs | fp8 cache = {m8:.3e}  16-bit cache = {m16:.3e}  ratio = {m8 / m16:.2f}")
    print(f"kv8 parity | logits rms     | fp8 cache = {r8:.3e}  16-bit cache = {r16:.3e}  ratio = {r8 / r16:.2f}")
    print(f"kv8 parity | top-1 agreement with the oracle | fp8 cache = {t8:.3f}  16-bit cache = {t16:.3f}  "
          f"decisive (step, row) pairs = {n8} of {(STEPS + 1) * B}")
    e8.set_kv_scales(torch.ones(LAYERS, 2, HEADS))
    m1, r1, _, _, t1 = teacher_forced(e8, world)
    print(f"kv8 parity | uncalibrated (scales 1.0) | max-abs = {m1:.3e}  rms = {r1:.3e}  top-1 = {t1:.3f}")
    assert m8 <= FACTOR * m16 and r8 <= FACTOR * r16, (m8, m16, r8, r16)
    assert a8 and a16 and n8 > 0


def test_graph_and_eager_agree_and_scales_are_data(world):
    eng, emb, pad = world["kv8"], world["emb"], world["pad"]
    eng.set_kv_scales(torch.ones(LAYERS, 2, HEADS))
    eng._graphs.clear()
    runs = {}
    for graph in (True, False):
        eng.prefill(emb, pad, STEPS + 2)
        assert eng.kv is not None and eng.kv.kc.dtype == torch.uint8 and eng.kv.kc.element_size() == 1
        runs[graph] = eng.decode(STEPS + 1, GREEDY, use_graph=graph, return_logits=True)
    assert runs[True][0].shape == (B, STEPS + 1) and torch.isfinite(runs[True][1]).all()
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])
    assert len(eng._graphs) == 1 and all(("kv", "fp8") in k for k in eng._graphs), "kv_dtype must be part of every graph key"
    # other scales: the same captured step, other logits (coarse scales on purpose)
    eng.set_kv_scales(pow2_table(1, 2, 5))
    eng.prefill(emb, pad, STEPS + 2)
    c2, l2 = eng.decode(STEPS + 1, GREEDY, use_graph=True, return_logits=True)
    assert len(eng._graphs) == 1
    assert not torch.equal(l2, runs[True][1])
    eng.set_kv_scales(torch.ones(LAYERS, 2, HEADS))
    for wrong in (torch.full((LAYERS, 2, HEADS), 3.0), torch.zeros(LAYERS, 2, HEADS), -torch.ones(LAYERS, 2, HEADS), torch.ones(LAYERS, 2)):
        with pytest.raises(ValueError):
            eng.set_kv_scales(wrong)
    # the 16-bit engine's keys carry ("kv", None)
    e16 = world["bf16"]
    e16._graphs.clear()
    e16.prefill(emb, pad, 6)
    e16.decode(4, GREEDY)
    assert e16._graphs and all(("kv", None) in k for k in e16._graphs)


def test_pool_bytes_export_and_accounting(world):
    from indextts.utils import quant
    e8, e16, emb, pad = world["kv8"], world["bf16"], world["emb"], world["pad"]
    e8.set_kv_scales(pow2_table(2))
    e8.prefill(emb, pad, STEPS)
    e16.prefill(emb, pad, STEPS)
    assert e8.kv.kc.element_size() == 1 and e16.kv.kc.element_size() == 2 and e8.kv.blocks == e16.kv.blocks and e8.kv.bs == e16.kv.bs
    pool = lambda e: e.kv.kc.numel() * e.kv.kc.element_size() + e.kv.vc.numel() * e.kv.vc.element_size()  # noqa: E731
    assert 2 * pool(e8) == pool(e16)
    S = emb.shape[1] + 1
    kc, vc = e8.dense_kv(B, S)
    k, v = e8.export_kv(B, S)
    sc = e8.kv_scale[:, :, None, :, None, None].double()
    assert kc.dtype == torch.uint8 and k.dtype == torch.float32
    assert torch.equal(k.double(), quant.decode_e4m3(kc) * sc[:, 0]) and torch.equal(v.double(), quant.decode_e4m3(vc) * sc[:, 1])
    # the prefill's codes are the host quantiser's of the 16-bit engine's keys (same kernels, same qkv), real positions only
    k16, v16 = e16.export_kv(B, S)
    for b, p in enumerate(world["pad"].tolist()):
        assert torch.equal(kc[:, b, :, p:], quant.quantize_kv_e4m3(k16[:, b, :, p:], sc[:, 0, 0]))
        assert torch.equal(vc[:, b, :, p:], quant.quantize_kv_e4m3(v16[:, b, :, p:], sc[:, 1, 0]))
    n8, b8 = e8.gemm_launches_of_step(B)
    n16, b16 = e16.gemm_launches_of_step(B)
    assert n8 == n16 == 4 * LAYERS + 1 and b8 == b16                  # the GEMMs move the same bytes; the cache is priced below
    ctx = 100
    assert e16.step_bytes(B, ctx) - e8.step_bytes(B, ctx) == (B * ctx + B) * LAYERS * 2 * D
    e8.set_kv_scales(torch.ones(LAYERS, 2, HEADS))


def test_composes_with_fp8_weights(world):
    eng, emb, pad = world["w8kv8"], world["emb"], world["pad"]
    eng.calibrate_kv_scales(emb, pad)
    out = {}
    for graph in (True, False):
        eng.prefill(emb, pad, STEPS + 2)
        out[graph] = eng.decode(STEPS + 1, GREEDY, use_graph=graph, return_logits=True)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1]) and torch.isfinite(out[True][1]).all()
    assert all(("kv", "fp8") in k and ("weights", "fp8") in k for k in eng._graphs) and eng.kv.kc.element_size() == 1


def test_calibration_leaves_no_saturated_code(world):
    """The synthetic prompt's |k|, |v| maxima are not powers of two (asserted), so with a headroom of 2 no stored code of the
    calibration prompt's own prefill is +-448."""
    eng, emb, pad = world["kv8"], world["emb"], world["pad"]
    sc = eng.calibrate_kv_scales(emb, pad).clone()
    from indextts.utils import quant
    assert bool(quant.is_pow2(sc.cpu()).all()) and not torch.equal(sc.cpu(), torch.ones(LAYERS, 2, HEADS))
    eng.prefill(emb, pad, 4)
    S = emb.shape[1] + 1
    kc, vc = eng.dense_kv(B, S)
    k, v = eng.export_kv(B, S)
    for b, p in enumerate(pad.tolist()):
        for codes in (kc, vc):
            assert int(((codes[:, b, :, p:] & 0x7F) == 0x7E).sum()) == 0
    amax = torch.stack([torch.stack([t[:, b, :, p:].abs().amax(dim=(2, 3)) for b, p in enumerate(pad.tolist())]).amax(0) for t in (k, v)], 1)
    assert bool((amax / sc <= 224.0 * 1.07).all()) and bool((amax / sc > 100.0).all())     # (decoded values: within one code of amax <= 224 s)
    eng.set_kv_scales(torch.ones(LAYERS, 2, HEADS))


def test_refill_over_two_slots_gives_the_static_batch_tokens(world):
    """Greedy, own-seed RowSampling rows; force_stop fixes every utterance's length, so the refill schedule does not depend on the
    tokens.  The entering rows' prompt K / V are quantised on the host (quant.quantize_kv_e4m3), bit-equal to itts_kv8_store."""
    eng, emb, pad = world["kv8"], world["emb"], world["pad"].tolist()
    eng.calibrate_kv_scales(world["emb"], world["pad"])
    stops = [5, 9, 3, 7]
    max_new, ce = 12, 4
    rows = [dict(GREEDY, seed=100 + i, stream=0) for i in range(B)]
    eng.prefill(world["emb"], world["pad"], max_new + ce)
    static = eng.decode(max_new, rows, force_stop=stops).cpu()
    queue = [2, 3]
    # slots 0 and 1 start with utterances 0 and 1 (their own left padding: the two-row batch is padded to its longer row)
    P = emb.shape[1]
    first = [emb[b, pad[b]:] for b in (0, 1)]
    L2 = max(int(f.shape[0]) for f in first)
    emb2 = torch.zeros(2, L2, D)
    pad2 = []
    for j, f in enumerate(first):
        emb2[j, L2 - f.shape[0]:] = f
        pad2.append(L2 - int(f.shape[0]))
    eng.prefill(emb2, torch.tensor(pad2, dtype=torch.int32), 200)

    def feed(k):
        take = [queue.pop(0) for _ in range(min(k, len(queue)))]
        return [(emb[i, pad[i]:].to(DEV), stops[i], rows[i]) for i in take]

    codes, leftover = eng.decode_refill(max_new, rows[:2], feed, force_stop=stops[:2], check_every=ce)
    assert not leftover and len(codes) == B and eng.refill_stats["rows_refilled"] == 2 and P > 0
    for i in range(B):
        want = static[i, : stops[i] + 1]
        assert torch.equal(codes[i].cpu(), want), (i, codes[i], want)
    eng.set_kv_scales(torch.ones(LAYERS, 2, HEADS))


def test_refusals(world, monkeypatch):
    from indextts.gpt.engine import GPTEngine
    eng, emb, pad, W = world["kv8"], world["emb"], world["pad"], world["W"]
    A, Bm = torch.zeros(4, D), torch.zeros(D, 4)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.prefill(emb, pad, 4, beams=3)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.prefill_beams(emb, pad, 4, 3)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.prefill(emb, pad, 4, paged=False)
    eng.prefill(emb, pad, 4)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.decode_beam(4, dict(GREEDY, length_penalty=0.0), 3)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.attach_lora({"gpt.h.0.attn.c_proj": (A, Bm)}, 1.0)
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.attach_lora_bank([({"gpt.h.0.attn.c_proj": (A, Bm)}, 1.0)])
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        eng.latent_mel_rows(torch.zeros(B * 3, D), [3] * B, cache_rows=list(range(B)))
    with pytest.raises(ValueError, match="16-bit"):
        GPTEngine(W, LAYERS, D, HEADS, dtype=torch.float32, device=DEV, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        GPTEngine(W, LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, kv_dtype="int8")
    with pytest.raises(ValueError, match="FP8 KV|kv_dtype"):
        world["bf16"].set_kv_scales(torch.ones(LAYERS, 2, HEADS))
    # shared_rows is accepted: the un-shared prefill runs and kv_share stays 0
    lg0 = eng.prefill(emb, pad, 4).clone()
    lg1 = eng.prefill(emb, pad, 4, shared_rows=32)
    assert torch.equal(lg0, lg1) and int(eng.kv_share.item()) == 0
    monkeypatch.setenv("ITTS_DECODE_MODE", "launch")
    with pytest.raises(ValueError, match="fold"):
        GPTEngine(W, LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, kv_dtype="fp8")
    monkeypatch.delenv("ITTS_DECODE_MODE")
    monkeypatch.setenv("ITTS_PAGED_KV", "0")
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        GPTEngine(W, LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, kv_dtype="fp8")
