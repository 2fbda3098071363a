"""FitEngine under FitConfig(attention="hip") on the small fp32 model and the three ragged utterances of
tests/test_fit_engine_gpu.py, against the float64 restatement of tests/fit_refs.py under that file's own rules: losses within 2e-3,
gradients and the 3-step trajectory within max(4 e32, 2^-18), the bf16 engine within its score gap.  The default arm is that file's
business; here it only serves as the other side of a printed comparison."""
import pytest
import torch

import fit_refs as FR
import test_fit_engine_gpu as TE
from test_fit_engine_gpu import cond_mel, ref, tts32  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FLOOR = TE.FLOOR


def engine(tts, **kw):
    return TE.engine(tts, attention="hip", **kw)


def test_step0_losses(tts32, ref):  # noqa: F811
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
    with torch.enable_grad():                          # evaluate: the same bits whatever the caller's grad mode
        on = fit.evaluate(b)
    with torch.no_grad():
        off = fit.evaluate(b)
    assert on == off == got


def test_gradients_against_float64_and_the_torch_arm(tts32, ref):  # noqa: F811
    sd, conds, m64, m32 = ref
    texts, codes = TE.ragged(FR.fixture())
    fit, plain = engine(tts32), TE.engine(tts32)
    assert fit.cfg.attention == "hip" and plain.cfg.attention == "torch"
    b = fit.batch(conds, texts, codes)
    f = TE.random_factors(sd)
    fit.set_factors(f)
    plain.set_factors(f)
    lh, lt = fit.backward(b), plain.backward(b)
    dev, other = fit.grads(), plain.grads()
    _, g64 = FR.loss_and_grads(m64, TE.ref_batch(b), f, 2.0, 0.1)
    _, g32 = FR.loss_and_grads(m32, TE.ref_batch(b), f, 2.0, 0.1)
    print(f"loss hip {float(lh['loss']):.7f}, torch {float(lt['loss']):.7f}, difference {abs(float(lh['loss']) - float(lt['loss'])):.3e}")
    for key in g64:
        for j in range(2):
            e32, ed, et = TE.rel(g32[key][j], g64[key][j]), TE.rel(dev[key][j], g64[key][j]), TE.rel(other[key][j], g64[key][j])
            print(f"{key} d{'AB'[j]}: e32 {e32:.3e}, hip {ed:.3e}, torch arm {et:.3e}, hip against torch {TE.rel(dev[key][j], other[key][j].cpu()):.3e}, "
                  f"allowed {max(4 * e32, FLOOR):.3e}")
            assert ed <= max(4 * e32, FLOOR), (key, j)
    fit.backward(b)                                    # the same bits on a second run
    again = fit.grads()
    assert all(torch.equal(again[k][j], dev[k][j]) for k in dev for j in range(2))


def test_an_utterance_gives_the_same_bits_alone_in_the_batch_and_reversed(tts32, ref):  # noqa: F811
    """An utterance's nll -- and what it hands back to its own rows: the gradient of its nll sum with respect to the first block's
    qkv rows, through both attention launches of every block -- alone, in the batch of three and in the batch reversed."""
    sd, conds, _, _ = ref
    texts, codes = TE.ragged(FR.fixture())
    fit = engine(tts32)
    fit.set_factors(TE.random_factors(sd))
    import indextts.gpt.fit as fitmod

    def run(ix):
        taps = []
        orig = fitmod._Attn.apply

        def tap(qkv, fe, rows):
            if not taps:
                qkv.retain_grad()
                taps.append((qkv, rows))
            return orig(qkv, fe, rows)
        fitmod._Attn.apply = tap
        try:
            with torch.enable_grad():
                o = fit._forward(fit.batch(conds, [texts[i] for i in ix], [codes[i] for i in ix]), False)
                (o["text_nll"].sum() + o["mel_nll"].sum()).backward()
        finally:
            del fitmod._Attn.apply                     # (the inherited classmethod again)
        qkv, rows = taps[0]
        out, at = {}, {"text": 0, "mel": 0}
        for slot, i in enumerate(ix):
            f, n = rows.segments[slot]
            out[(i, "dqkv")] = qkv.grad[f: f + n].clone()
            for name in ("text", "mel"):
                k = (texts[i] if name == "text" else codes[i]).numel() + 2
                out[(i, name)] = o[f"{name}_nll"][at[name]: at[name] + k].detach().clone()
                at[name] += k
        return out
    batch, back = run([0, 1, 2]), run([2, 1, 0])
    for i in range(3):
        alone = run([i])
        for what in ("text", "mel", "dqkv"):
            assert alone[(i, what)].abs().max() > 0
            assert torch.equal(alone[(i, what)], batch[(i, what)]) and torch.equal(alone[(i, what)], back[(i, what)]), (i, what)


def test_three_steps_follow_the_float64_trajectory(tts32, ref):  # noqa: F811
    sd, conds, m64, m32 = ref
    texts, codes = TE.ragged(FR.fixture())
    c = FR.OVERFIT
    kw = dict(lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    fit = engine(tts32, **kw)
    b = fit.batch(conds, texts, codes)
    t64, t32 = FR.Trainer(m64, FR.init_factors(sd, 2, 4, 0), 2.0, **kw), FR.Trainer(m32, FR.init_factors(sd, 2, 4, 0), 2.0, **kw)
    for _ in range(3):
        rd, r64 = fit.step(b), t64.step(TE.ref_batch(b))
        t32.step(TE.ref_batch(b))
        assert abs(rd["loss_mel"] - r64["loss_mel"]) <= 2e-3 and abs(rd["loss_text"] - r64["loss_text"]) <= 2e-3
    ad, _ = fit.voice()
    worst = []
    for key in ad:
        for j in range(2):
            e32, ed = TE.rel(t32.f[key][j], t64.f[key][j]), TE.rel(ad[key][j], t64.f[key][j])
            print(f"{key} {'AB'[j]} after 3 steps: e32 {e32:.3e}, device {ed:.3e}, allowed {max(4 * e32, FLOOR):.3e}")
            if ed > max(4 * e32, FLOOR):
                worst.append((key, "AB"[j], e32, ed))
    assert not worst, worst


def test_a_torch_arm_state_dict_loads_and_steps(tts32, ref):  # noqa: F811
    _, conds, _, _ = ref
    texts, codes = TE.ragged(FR.fixture())
    plain = TE.engine(tts32, lr=1e-3)
    b = plain.batch(conds, texts, codes)
    plain.step(b), plain.step(b)
    sd = plain.state_dict()
    assert "attention" not in sd and all(torch.is_tensor(v) or isinstance(v, (int, float)) for v in sd.values())
    fit = engine(tts32, lr=1e-3)
    assert sorted(fit.state_dict()) == sorted(sd)
    fit.load_state_dict(sd)
    a = fit.voice()[0]
    assert all(torch.equal(a[k][j], plain.voice()[0][k][j]) for k in a for j in range(2))
    rep = fit.step(b)
    assert rep["step"] == 3 and rep["loss_mel"] > 0 and rep["grad_norm"] > 0
    assert any(not torch.equal(fit.voice()[0][k][1], a[k][1]) for k in a)


def test_fit_voice_passes_attention_through(tts32, cond_mel):  # noqa: F811
    texts, codes = TE.ragged(FR.fixture())
    with pytest.raises(ValueError, match="attention must be one of"):
        tts32.fit_voice(cond_mel, texts, codes, steps=1, attention="cuda")
    adapters, scaling, report = tts32.fit_voice(cond_mel, texts, codes, steps=2, lr=1e-3, dropout=0.0, return_report=True, attention="hip")
    assert scaling == 2.0 and len(adapters) == 8 and len(report["steps"]) == 2


def test_bf16_engine_step(cond_mel):  # noqa: F811
    """One step of a bf16 engine under "hip" against the float64 trajectory's first step within the existing bf16 test's gap."""
    tts = TE.make_tts("bf16")
    sd = TE.gpt_state()
    texts, codes = TE.ragged(FR.fixture())
    conds = tts._prompt_features(cond_mel, spk=False)[0].detach()
    c = FR.OVERFIT
    kw = dict(lr=c["lr"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    fit = engine(tts, **kw)
    b = fit.batch(conds, texts, codes)
    t64 = FR.Trainer(FR.Model(sd, 2), FR.init_factors(sd, 2, 4, 0), 2.0, **kw)
    rd, r64 = fit.step(b), t64.step(TE.ref_batch(b))
    print(f"bf16 step: loss_mel {rd['loss_mel']:.4f} (float64 {r64['loss_mel']:.4f}), loss_text {rd['loss_text']:.4f} ({r64['loss_text']:.4f})")
    assert abs(rd["loss_mel"] - r64["loss_mel"]) <= TE.BF16_GAP and abs(rd["loss_text"] - r64["loss_text"]) <= TE.BF16_GAP
