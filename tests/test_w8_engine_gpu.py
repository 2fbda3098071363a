"""The FP8-weight decode engine (GPTEngine(weight_dtype="fp8")) end to end on the small synthetic GPT (2 layers, full width): its
logits and latents against oracle/gpt_ref.py run on the DEQUANTISED weights, with the bf16 engine built from those same weights
as the yardstick; paged / contiguous, graph / eager and beam self-consistency; accounting and refusals; the public surface.

The FP8 engine is built from the ORIGINAL state dict W (LayerNorm gamma = 1 + 0.1 u, beta = 0.02 u, tests/synth.py): it folds gamma
into the QKV / FC weights before it quantises them, forms d = beta W + b, and runs its prefill and latent passes as LayerNorm
without affine over the dequantised gamma . W.  The oracle and the bf16 yardstick run on Wd = quant.dequantized_gpt_weights(W), the
model those steps must add up to (the same scale . code values, stored fp32): a wrong d, a dropped beta or a prefill that kept the
original gamma is an error of the size of the logits, not of the bound.

Parity rule.  The FP8 engine's weights are exact where the bf16 engine rounds scale . code to bf16, so against the oracle over the
dequantised weights its error should not be larger than the bf16 engine's: err_fp8 <= 1.25 x err_bf16 + 1e-6 on max-abs logits
(and latents); the 1.25 covers another summation order.  Measured on an MI355X (profiles/w8_engine_parity.txt):
    logits  err_fp8 = 3.036e-02  err_bf16 = 3.256e-02        latents  err_fp8 = 1.731e-02  err_bf16 = 1.731e-02
(the latent pass runs over the same 16-bit copies of the dequantised weights in both engines: equal bits, equal error)."""
import numpy as np
import pytest
import torch

import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS, D, HEADS, STEPS = 2, 1280, 20, 6
GREEDY = dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=10.0, seed=0)


@pytest.fixture(scope="module")
def world():
    """The dequantised state dict (fp32, CPU), the two engines built from it, the prompt and the oracle's teacher-forced trace:
    computed once, shared, left unchanged."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts.gpt.engine import GPTEngine
    from indextts.utils import quant
    from oracle import gpt_ref
    W = {k: v.float() for k, v in weights.gpt_state_dict(LAYERS, with_conditioner=False).items()}
    Wd = quant.dequantized_gpt_weights(W, LAYERS)
    g = torch.Generator().manual_seed(3)
    conds = torch.randn(1, 32, D, generator=g) * 0.5
    rng = np.random.default_rng(7)
    text = torch.ones(3, 11, dtype=torch.int64)                       # unequal lengths: right-padded with the stop token (1)
    for b, n in enumerate((11, 4, 8)):
        text[b, :n] = torch.from_numpy(rng.integers(2, 12000, size=n))
    emb, mask, pad = gpt_ref.prepare_gpt_inputs(conds, text, Wd)
    lg, past = gpt_ref.decode_prefill(emb, mask, Wd)
    ref_logits, toks = [lg], []
    for s in range(1, STEPS + 1):
        tok = lg.argmax(-1)
        toks.append(tok)
        mask = torch.cat([mask, torch.ones(3, 1, dtype=torch.bool)], 1)
        lg, past = gpt_ref.decode_step(tok, s, mask, past, Wd)
        ref_logits.append(lg)
    lat_emb = torch.randn(2, 9, D, generator=g) * 0.5
    hidden, _ = gpt_ref.transformer(lat_emb, Wd, torch.ones(2, 9, dtype=torch.bool))
    ref_lat = gpt_ref.layer_norm(hidden, Wd["final_norm.weight"], Wd["final_norm.bias"])
    mk = lambda sd, wd: GPTEngine(sd, LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, weight_dtype=wd)  # noqa: E731
    return dict(Wd=Wd, emb=emb, pad=pad.to(torch.int32), ref_logits=ref_logits, toks=toks, lat_emb=lat_emb, ref_lat=ref_lat,
                fp8=mk(W, "fp8"), bf16=mk(Wd, None))


def teacher_forced_error(eng, w):
    """max-abs logit error over the prefill and STEPS decode steps, the oracle's greedy tokens forced."""
    lg = eng.prefill(w["emb"], w["pad"], STEPS + 2)
    errs = [(lg.cpu() - w["ref_logits"][0]).abs().max().item()]
    for s in range(1, STEPS + 1):
        eng._sample(3, GREEDY)
        eng.tokens[:3] = w["toks"][s - 1].to(torch.int32).to(DEV)
        eng.history[:3, s - 1] = eng.tokens[:3]
        eng._step_transformer(3)
        errs.append((eng.logits[:3].cpu() - w["ref_logits"][s]).abs().max().item())
    return max(errs)


def test_logits_and_latents_against_the_oracle_on_the_dequantised_weights(world):
    e8, e16 = teacher_forced_error(world["fp8"], world), teacher_forced_error(world["bf16"], world)
    print(f"w8 parity | logits  | err_fp8 = {e8:.3e}  err_bf16 = {e16:.3e}")
    l8 = (world["fp8"].latent(world["lat_emb"]).cpu() - world["ref_lat"]).abs().max().item()
    l16 = (world["bf16"].latent(world["lat_emb"]).cpu() - world["ref_lat"]).abs().max().item()
    print(f"w8 parity | latents | err_fp8 = {l8:.3e}  err_bf16 = {l16:.3e}")
    assert e8 <= 1.25 * e16 + 1e-6, (e8, e16)
    assert l8 <= 1.25 * l16 + 1e-6, (l8, l16)


def test_paged_graph_and_beam_forms_agree_bit_for_bit(world):
    eng, emb, pad = world["fp8"], world["emb"], world["pad"]
    runs = {}
    for name, paged, graph in (("paged-graph", True, True), ("paged-eager", True, False), ("contiguous-graph", False, True)):
        eng._graphs.clear()
        eng.prefill(emb, pad, STEPS + 2, paged=paged)
        assert (eng.kv is not None) == paged
        runs[name] = eng.decode(STEPS + 1, GREEDY, use_graph=graph, return_logits=True)
    c0, l0 = runs["paged-graph"]
    assert c0.shape == (3, STEPS + 1) and torch.isfinite(l0).all()
    for name in ("paged-eager", "contiguous-graph"):
        assert torch.equal(runs[name][0], c0) and torch.equal(runs[name][1], l0), name
    assert eng._graphs and all(("weights", "fp8") in k for k in eng._graphs), "weight_dtype must be part of every graph key"
    beams = []
    for graph in (True, False):
        eng._graphs.clear()
        eng.prefill_beams(emb, pad, STEPS + 2, 3)
        beams.append(eng.decode_beam(STEPS + 1, dict(GREEDY, length_penalty=0.0), 3, use_graph=graph))
    assert beams[0].shape[0] == 3 and torch.equal(beams[0], beams[1])
    eng._graphs.clear()


def test_accounting_and_refusals(world, monkeypatch):
    from indextts.gpt.engine import GPTEngine
    e8, e16 = world["fp8"], world["bf16"]
    assert abs(e8.weight_bytes - e16.weight_bytes / 2) <= 0.01 * e16.weight_bytes / 2, (e8.weight_bytes, e16.weight_bytes)
    e8.prefill(world["emb"], world["pad"], 4)
    n8, b8 = e8.gemm_launches_of_step(3)
    e16.prefill(world["emb"], world["pad"], 4)
    n16, b16 = e16.gemm_launches_of_step(3)
    assert n8 == n16 == 4 * LAYERS + 1 and b16 - b8 == LAYERS * 12 * D * D + e8.V * D      # one byte per weight is what is priced
    A, B = torch.zeros(4, D), torch.zeros(D, 4)
    with pytest.raises(ValueError, match="FP8"):
        e8.attach_lora({"gpt.h.0.attn.c_proj": (A, B)}, 1.0)
    with pytest.raises(ValueError, match="FP8"):
        e8.attach_lora_bank([({"gpt.h.0.attn.c_proj": (A, B)}, 1.0)])
    with pytest.raises(ValueError, match="16-bit"):
        GPTEngine(world["Wd"], LAYERS, D, HEADS, dtype=torch.float32, device=DEV, weight_dtype="fp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        GPTEngine(world["Wd"], LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, weight_dtype="int8")
    monkeypatch.setenv("ITTS_DECODE_MODE", "launch")
    with pytest.raises(ValueError, match="fold"):
        GPTEngine(world["Wd"], LAYERS, D, HEADS, dtype=torch.bfloat16, device=DEV, weight_dtype="fp8")


def test_public_surface_serves_fp8_and_keeps_int8_on_bf16(capsys):
    import synth
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = LAYERS
    sd, bsd = weights.gpt_state_dict(LAYERS), weights.bigvgan_state_dict()
    tts = IndexTTS.from_weights(cfg, sd, bsd, device="cuda:0", precision_config={"gpt": "fp8", "vocoder": "fp16"})
    assert "GPT=bf16 activations / e4m3 weights" in capsys.readouterr().out
    assert tts.gpt_weight_dtype == "fp8" and tts.gpt_dtype == torch.bfloat16 and tts.gpt.engine.weight_dtype == "fp8"
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    rows = [torch.tensor([11, 22, 33, 44, 55]), torch.tensor([66, 77, 88])]
    gen = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1)
    wavs, codes = tts.infer_batch(cond_mel, rows, max_mel_tokens=9, force_stop=[8, 6], seed=5, return_codes=True, **gen)
    assert [int(c.numel()) for c in codes] == [8, 6]
    for w, n in zip(wavs, (8, 6)):
        assert w.numel() == n * 1024 and torch.isfinite(w.float()).all() and w.float().abs().max().item() > 0
    del tts
    int8 = IndexTTS.from_weights(cfg, sd, bsd, device="cuda:0", precision_config={"gpt": "int8", "vocoder": "fp16"})
    assert "bitsandbytes quantisation is not available" in capsys.readouterr().out
    assert int8.gpt_weight_dtype is None and int8.gpt_dtype == torch.bfloat16 and int8.gpt.engine.weight_dtype is None
    assert int8.gpt.engine.s_head is None
