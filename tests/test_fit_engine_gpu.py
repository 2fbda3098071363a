"""Voice fitting end to end on the device (indextts/gpt/fit.py, IndexTTS.fit_voice) on the small fp32 model
of tests/test_score_engine_gpu.py and three ragged utterances of tests/golden/score_small.npz (9 / 4 / 6 codes), against the float64
restatement of tests/fit_refs.py.  The tolerance of a gradient or a trajectory is MEASURED against that reference, not fixed: the same
graph in fp32 torch on the CPU gives e32 = max |g32 - g64| / max |g64| per factor, and the device may err 4 e32, floored at 2^-18
(the factor 4 because the summation orders differ)."""
import pytest
import torch

import fit_refs as FR
import synth
import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -18
BF16_GAP = 0.33     # the bf16 score gap of tests/test_score_engine_gpu.py (see test_bf16_engine_steps)


def gpt_state():
    sd = dict(weights.gpt_state_dict(2))
    sd.update({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({"text_head.weight": (12001, 1280), "text_head.bias": (12001,)},
                                                                         synth.gpt_param).items()})
    return sd


def make_tts(gpt="fp32"):
    from indextts.infer import IndexTTS
    cfg = weights.reference_config()
    cfg["gpt"]["layers"] = 2
    return IndexTTS.from_weights(cfg, gpt_state(), weights.bigvgan_state_dict(), device="cuda:0",
                                 precision_config=dict(gpt=gpt, vocoder="fp32" if gpt == "fp32" else "fp16"))


@pytest.fixture(scope="module")
def tts32():
    return make_tts()


@pytest.fixture(scope="module")
def cond_mel():
    return torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)


def ragged(fx):
    texts = [torch.from_numpy(fx["text"][i, : int(fx["text_lens"][i])]) for i in range(3)]
    codes = [torch.from_numpy(fx["codes"][i, :n]) for i, n in enumerate((9, 4, 6))]
    return texts, codes


@pytest.fixture(scope="module")
def ref(tts32, cond_mel):
    """The float64 side, computed once: (state dict, conds on the device, float64 model, fp32 model, the ragged batch as the
    reference takes it)."""
    sd = gpt_state()
    conds = tts32._prompt_features(cond_mel, spk=False)[0].detach()      # what score_codes and fit_voice condition on
    return sd, conds, FR.Model(sd, 2), FR.Model(sd, 2, torch.float32)


def engine(tts, **kw):
    from indextts.gpt.fit import FitConfig, FitEngine
    c = dict(rank=4, alpha=8.0, dropout=0.0)
    c.update(kw)
    return FitEngine(tts.gpt.engine, tts.gpt._sd, FitConfig(**c))


def ref_batch(b):
    """A FitEngine batch as tests/fit_refs.py takes it (FR.batch_losses): the padded tuple, or the ragged dict with conds on the CPU."""
    if "text_rows" in b:
        return dict(b, conds=b["conds"].cpu())
    return tuple(b[k].cpu() for k in ("conds", "text", "text_lengths", "codes", "wav_lengths"))


def random_factors(sd, seed=5, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return {k: (A, torch.randn(B.shape, generator=g) * std) for k, (A, B) in FR.init_factors(sd, 2, 4, seed).items()}


def rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def test_step0_losses_are_score_and_the_fixture(tts32, cond_mel, ref):
    fx = FR.fixture()
    fit = engine(tts32)
    conds = ref[1]
    b = dict(conds=conds, text=torch.from_numpy(fx["text"]), text_lengths=torch.from_numpy(fx["text_lens"]),
             codes=torch.from_numpy(fx["codes"]), wav_lengths=torch.from_numpy(fx["wav_lengths"]))
    got = fit.evaluate(b)
    sc = tts32.gpt.score(None, b["text"], b["text_lengths"], b["codes"], b["wav_lengths"], conds=conds)
    for name in ("text", "mel"):
        print(name, got[f"loss_{name}"], sc[f"loss_{name}"].item(), float(fx[f"loss_{name}_64"]))
        assert abs(got[f"loss_{name}"] - sc[f"loss_{name}"].item()) <= 2e-3
        assert abs(got[f"loss_{name}"] - float(fx[f"loss_{name}_64"])) <= 2e-3


def test_gradients_against_float64(tts32, ref):
    sd, conds, m64, m32 = ref
    texts, codes = ragged(FR.fixture())
    fit = engine(tts32)
    b = fit.batch(conds, texts, codes)
    f = random_factors(sd)
    fit.set_factors(f)
    fit.backward(b)
    dev = fit.grads()
    _, g64 = FR.loss_and_grads(m64, ref_batch(b), f, 2.0, 0.1)
    _, g32 = FR.loss_and_grads(m32, ref_batch(b), f, 2.0, 0.1)
    for key in g64:
        for j in range(2):
            e32, ed = rel(g32[key][j], g64[key][j]), rel(dev[key][j], g64[key][j])
            print(f"{key} d{'AB'[j]}: e32 {e32:.3e}, device {ed:.3e}, allowed {max(4 * e32, FLOOR):.3e}")
            assert ed <= max(4 * e32, FLOOR), (key, j)
    # B = 0: every dA is exactly zero, every dB is not
    fit.set_factors(FR.init_factors(sd, 2, 4, 0))
    fit.backward(b)
    for key, (dA, dB) in fit.grads().items():
        assert not dA.any() and dB.abs().max() > 0, key


def test_accumulation_over_two_half_batches_is_the_whole_batch(tts32, ref):
    """The three utterances as two micro-batches -- [0, 1] and [2], each another rectangle -- weighted per head by their share of the
    whole batch's positions (a loss is a mean over positions), against the whole batch in one backward.  The bound is
    ittf_lora_wgrad's own, from the operands of the runs themselves (FitEngine.probe): per entry 2^-24 times the sum over the three
    reductions of (M + 2) sum_m |s z|, plus one rounding of the accumulated G.  (An utterance's rows give the same bits in either
    rectangle -- the test below -- so the reductions differ in their order alone.)"""
    sd, conds, _, _ = ref
    texts, codes = ragged(FR.fixture())
    fit = engine(tts32)
    fit.set_factors(random_factors(sd))
    fit.probe = {}
    whole_b = fit.batch(conds, texts, codes)
    fit.backward(whole_b)
    whole = fit.grads()
    nt, nm = [t.numel() + 2 for t in texts], [c.numel() + 2 for c in codes]
    parts = ([0, 1], [2])
    for k, ix in enumerate(parts):
        b = fit.batch(conds, [texts[i] for i in ix], [codes[i] for i in ix])
        fit.backward(b, accumulate=k > 0, head_weights=(sum(nt[i] for i in ix) / sum(nt), sum(nm[i] for i in ix) / sum(nm)))
    halves = fit.grads()
    worst = 0.0
    for key, runs in fit.probe.items():
        assert len(runs) == 3
        bound_a = sum((M + 2) * FR.U * ma for M, ma, _ in runs).cpu()
        bound_b = sum((M + 2) * FR.U * mb for M, _, mb in runs).cpu()
        for got, want, bound in ((halves[key][0], whole[key][0], bound_a), (halves[key][1].t(), whole[key][1].t(), bound_b)):
            err = (got.double().cpu() - want.double().cpu()).abs()
            bound = bound + FR.U * want.double().cpu().abs()
            assert (err <= bound).all(), (key, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"two half-batches against the whole batch: worst |difference| / bound {worst:.3e}")
    fit.probe = None
    fit.backward(whole_b)                              # and the same bits on a second run
    again = fit.grads()
    assert all(torch.equal(again[k][j], whole[k][j]) for k in whole for j in range(2))


def test_an_utterance_contributes_the_same_bits_alone_and_in_the_batch(tts32, ref):
    """What an utterance contributes to a loss is its positions' nll: the same bits evaluated alone, in the batch of three and in
    the batch reversed (other rectangles, other row offsets).  And its gradient alone equals its share of a batch of two copies of
    itself bit for bit only up to the reduction order, which the test above bounds."""
    sd, conds, _, _ = ref
    texts, codes = ragged(FR.fixture())
    fit = engine(tts32)
    fit.set_factors(random_factors(sd))

    def nll(ix):
        with torch.no_grad():
            o = fit._forward(fit.batch(conds, [texts[i] for i in ix], [codes[i] for i in ix]), False)
        out, at = {}, {"text": 0, "mel": 0}
        for i in ix:
            for name in ("text", "mel"):
                n = (texts[i] if name == "text" else codes[i]).numel() + 2
                out[(i, name)] = o[f"{name}_nll"][at[name]: at[name] + n].clone()
                at[name] += n
        return out
    batch, back = nll([0, 1, 2]), nll([2, 1, 0])
    for i in range(3):
        alone = nll([i])
        for name in ("text", "mel"):
            d1, d2 = (alone[(i, name)] - batch[(i, name)]).abs().max().item(), (alone[(i, name)] - back[(i, name)]).abs().max().item()
            print(f"utterance {i} {name}: max |nll alone - in the batch| {d1:.3e}, - in the batch reversed {d2:.3e}")
            assert torch.equal(alone[(i, name)], batch[(i, name)]) and torch.equal(alone[(i, name)], back[(i, name)]), (i, name)


def three_steps(tts32, ref):
    sd, conds, m64, m32 = ref
    texts, codes = ragged(FR.fixture())
    c = FR.OVERFIT
    fit = engine(tts32, lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    b = fit.batch(conds, texts, codes)
    kw = dict(lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    t64, t32 = FR.Trainer(m64, FR.init_factors(sd, 2, 4, 0), 2.0, **kw), FR.Trainer(m32, FR.init_factors(sd, 2, 4, 0), 2.0, **kw)
    reps = []
    for _ in range(3):
        reps.append((fit.step(b), t64.step(ref_batch(b))))
        t32.step(ref_batch(b))
    return fit, t64, t32, reps


def test_three_steps_report_the_float64_losses_norms_and_rates(tts32, ref):
    """Per step the device's loss_text / loss_mel within section 4.27's 2e-3 of the float64 trajectory's, the gradient norm within
    1e-3 of it (relative) and the same learning rate."""
    _, _, _, reps = three_steps(tts32, ref)
    for rd, r64 in reps:
        print(f"step {rd['step']}: loss_mel {rd['loss_mel']:.6f} ({r64['loss_mel']:.6f}), grad_norm {rd['grad_norm']:.6f} ({r64['grad_norm']:.6f})")
        assert abs(rd["lr"] - r64["lr"]) <= 1e-12 and abs(rd["loss_mel"] - r64["loss_mel"]) <= 2e-3 and abs(rd["loss_text"] - r64["loss_text"]) <= 2e-3
        assert abs(rd["grad_norm"] - r64["grad_norm"]) <= 1e-3 * r64["grad_norm"]


def test_three_steps_follow_the_float64_trajectory(tts32, ref):
    """The factors after 3 optimizer steps against the float64 trajectory's, under the measured rule of the gradients (4 e32,
    floored at 2^-18).
    What it is sensitive to: Adam's first updates divide a gradient by its own magnitude -- with two or three gradients in the
    moments the update is close to lr sign(g), and at step 3 every dA is seen for the first time (B was zero before) -- so a factor's
    error after 3 steps is the gradient's ABSOLUTE error over the size of its small entries, and e32 itself spans 9.4e-8 .. 2.1e-2
    over the factors on gradients good to 1e-6.  With every GEMM of the fit summed as one chain over K the device was outside on
    three factors whose reductions run over 5 120 elements (h.0.mlp.c_proj A 4.4e-5 against an allowed 1.3e-5, its B 8.2e-4 against
    4.5e-4, h.1.mlp.c_fc B 4.7e-3 against 3.9e-3; three fp32 runs on the CPU, 8 threads / 1 thread / the batch reversed, stay within
    3x of one another); with the reductions cut into slices of 256 (gpt/fit.py, _mm) all sixteen are inside, the worst at 0.59 of
    what is allowed (profiles/fit.txt)."""
    fit, t64, t32, _ = three_steps(tts32, ref)
    ad, _ = fit.voice()
    worst = []
    for key in ad:
        for j in range(2):
            e32, ed = rel(t32.f[key][j], t64.f[key][j]), rel(ad[key][j], t64.f[key][j])
            print(f"{key} {'AB'[j]} after 3 steps: e32 {e32:.3e}, device {ed:.3e}, allowed {max(4 * e32, FLOOR):.3e}")
            if ed > max(4 * e32, FLOOR):
                worst.append((key, "AB"[j], e32, ed))
    assert not worst, worst


def test_overfit_and_served_equals_trained(tts32, cond_mel, ref):
    """The test that matters most: the voice the fit returns, served through the pool, scores the training set as the fit's own last
    evaluation does (section 4.27's fp32 bound, 2e-3); without an adapter the step-0 losses come back."""
    sd, conds, m64, _ = ref
    texts, codes = ragged(FR.fixture())
    c = FR.OVERFIT
    fit = engine(tts32, lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    b = fit.batch(conds, texts, codes)
    start = fit.evaluate(b)
    kw = dict(lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    t64, t32 = FR.Trainer(m64, FR.init_factors(sd, 2, 4, 0), 2.0, **kw), FR.Trainer(ref[3], FR.init_factors(sd, 2, 4, 0), 2.0, **kw)
    for _ in range(c["steps"]):
        fit.step(b)
        t64.step(ref_batch(b))
        t32.step(ref_batch(b))
    last = fit.evaluate(b)
    with torch.no_grad():
        want = float(FR.batch_losses(m64, ref_batch(b), factors=t64.f, scaling=2.0)["loss_mel"])
        want32 = float(FR.batch_losses(ref[3], ref_batch(b), factors=t32.f, scaling=2.0)["loss_mel"])
    # the measured rule of the gradients on the final loss: e32 = the fp32 trajectory's relative distance from float64's
    e32, ed = abs(want32 - want) / want, abs(last["loss_mel"] - want) / want
    print(f"overfit: loss_mel {start['loss_mel']:.4f} -> {last['loss_mel']:.6f} (float64: {want:.6f}, fp32 on the CPU: {want32:.6f}); "
          f"e32 {e32:.3e}, device {ed:.3e}, allowed {max(4 * e32, FLOOR):.3e}")
    assert last["loss_mel"] < 0.5 * start["loss_mel"]
    assert ed <= max(4 * e32, FLOOR)
    base = tts32.score_codes(cond_mel, texts, codes)
    ids = tts32.attach_voice_pool(slots=2, rank=4)
    try:
        vid = tts32.add_voice(*fit.voice())
        served = tts32.score_codes(cond_mel, texts, codes, adapter_ids=[vid] * 3)
        plain = tts32.score_codes(cond_mel, texts, codes, adapter_ids=None)
    finally:
        tts32.detach_voice_pool()
    assert ids == []
    for i in range(3):
        print(i, served[i]["nll_mel"], last["nll_mel"][i], served[i]["nll_text"], last["nll_text"][i])
        assert abs(served[i]["nll_mel"] - last["nll_mel"][i]) <= 2e-3 and abs(served[i]["nll_text"] - last["nll_text"][i]) <= 2e-3
        assert abs(plain[i]["nll_mel"] - start["nll_mel"][i]) <= 2e-3 and abs(base[i]["nll_mel"] - start["nll_mel"][i]) <= 2e-3
        assert abs(served[i]["nll_mel"] - base[i]["nll_mel"]) > 0.5


def test_dropout_is_seeded_and_evaluation_never_drops(tts32, ref):
    sd, conds, _, _ = ref
    texts, codes = ragged(FR.fixture())
    runs = []
    for seed in (1, 1, 2):
        fit = engine(tts32, dropout=0.2, seed=seed, lr=1e-3)
        fit.set_factors(random_factors(sd))
        b = fit.batch(conds, texts, codes)
        ev = fit.evaluate(b)
        assert ev == fit.evaluate(b)
        fit.step(b)
        runs.append((ev, fit.grads()))
    same = lambda x, y: all(torch.equal(x[k][j], y[k][j]) for k in x for j in range(2))   # noqa: E731
    assert same(runs[0][1], runs[1][1]) and not same(runs[0][1], runs[2][1])
    assert runs[0][0] == runs[2][0]                    # the evaluation does not see the seed's masks (the same factors were set)


def test_resume_is_bit_equal(tts32, ref):
    _, conds, _, _ = ref
    texts, codes = ragged(FR.fixture())
    one = engine(tts32, lr=1e-3, dropout=0.2)
    b = one.batch(conds, texts, codes)
    for _ in range(3):
        one.step(b)
    two = engine(tts32, lr=1e-3, dropout=0.2)
    two.step(b), two.step(b)
    sd = two.state_dict()
    assert all(torch.is_tensor(v) or isinstance(v, (int, float)) for v in sd.values())
    three = engine(tts32, lr=1e-3, dropout=0.2)
    three.load_state_dict(sd)
    three.step(b)
    a, c = one.voice()[0], three.voice()[0]
    assert all(torch.equal(a[k][j], c[k][j]) for k in a for j in range(2)) and three.step_count == 3


def test_fit_voice_save_merged_round_trip_and_engine_state(tts32, cond_mel, tmp_path):
    """IndexTTS.fit_voice on the ragged rows; save_merged then voice_from_checkpoint recovers a voice that scores within 2e-3 of
    the fitted one; the engine's bank and an infer_batch before and after are unchanged."""
    texts, codes = ragged(FR.fixture())
    eng = tts32.gpt.engine
    gen = dict(max_mel_tokens=12, return_codes=True, do_sample=False, num_beams=1, repetition_penalty=1.0)
    _, before = tts32.infer_batch(cond_mel, [texts[0]], **gen)
    graphs = set(eng._graphs)
    c = FR.OVERFIT
    with pytest.raises(ValueError, match="too small for the longest utterance"):
        tts32.fit_voice(cond_mel, texts, codes, steps=1, batch_rows=40)
    adapters, scaling, report = tts32.fit_voice(cond_mel, texts, codes, steps=c["steps"], lr=c["lr"], batch_rows=4096, dropout=0.0,
                                                 return_report=True)
    assert scaling == 2.0 and len(adapters) == 8 and len(report["steps"]) == c["steps"]
    assert report["steps"][-1]["loss_mel"] < 0.5 * report["steps"][0]["loss_mel"]
    assert eng.bank is None and not eng.lora and set(eng._graphs) == graphs
    _, after = tts32.infer_batch(cond_mel, [texts[0]], **gen)
    assert torch.equal(before[0], after[0])
    path = tts32.save_merged(str(tmp_path / "gpt_finetuned.pth"), adapters, scaling)
    rec, rec_scaling = tts32.voice_from_checkpoint(path)
    tts32.attach_voice_pool([(adapters, scaling), (rec, rec_scaling)], slots=2, rank=16)
    try:
        fitted = tts32.score_codes(cond_mel, texts, codes, adapter_ids=[0] * 3)
        back = tts32.score_codes(cond_mel, texts, codes, adapter_ids=[1] * 3)
    finally:
        tts32.detach_voice_pool()
    for i in range(3):
        print(i, fitted[i]["nll_mel"], back[i]["nll_mel"])
        assert abs(fitted[i]["nll_mel"] - back[i]["nll_mel"]) <= 2e-3 and abs(fitted[i]["nll_text"] - back[i]["nll_text"]) <= 2e-3


def test_bf16_engine_steps(cond_mel):
    """A bf16 engine's loss_text and loss_mel at every one of six steps against the float64 trajectory's, within BF16_GAP: the
    figure tests/test_score_engine_gpu.py::test_bf16_head_meets_the_decode_path states for bf16 scores on this model (an nll
    difference of up to 0.33 at a position, which bounds the difference of means over positions).  It is that test's figure, not
    one fitted here: the differences measured on an MI355X are 2.0e-3 .. 4.6e-3 (loss_mel) and up to 9e-4 (loss_text)."""
    tts = make_tts("bf16")
    sd = gpt_state()
    texts, codes = ragged(FR.fixture())
    conds = tts._prompt_features(cond_mel, spk=False)[0].detach()
    c = FR.OVERFIT
    fit = engine(tts, lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    b = fit.batch(conds, texts, codes)
    t64 = FR.Trainer(FR.Model(sd, 2), FR.init_factors(sd, 2, 4, 0), 2.0, lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    for k in range(6):
        rd, r64 = fit.step(b), t64.step(ref_batch(b))
        print(f"bf16 step: loss_mel {rd['loss_mel']:.4f} (float64 {r64['loss_mel']:.4f}), loss_text {rd['loss_text']:.4f} ({r64['loss_text']:.4f})")
        assert abs(rd["loss_mel"] - r64["loss_mel"]) <= BF16_GAP and abs(rd["loss_text"] - r64["loss_text"]) <= BF16_GAP, k
        if k == 0:
            first = rd["loss_mel"]
    assert rd["loss_mel"] < first
