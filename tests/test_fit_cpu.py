"""Voice fitting without a device: the reference's own properties on the float64 restatement
(tests/fit_refs.py) -- its anchor on the reference's fixture, gradients against finite differences, the optimizer against
torch.optim.AdamW, the schedule, the B = 0 start, the overfit budget the device test relies on -- and every host refusal."""
import math

import pytest
import torch

import fit_refs as FR
import synth
import weights


def gpt_state():
    sd = dict(weights.gpt_state_dict(2))
    sd.update({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({"text_head.weight": (12001, 1280), "text_head.bias": (12001,)},
                                                                         synth.gpt_param).items()})
    return sd


@pytest.fixture(scope="module")
def ref():
    """(state dict, float64 model, conds, the fixture's padded batch, the ragged batch of 9 / 4 / 6 codes)"""
    sd = gpt_state()
    fx = FR.fixture()
    conds = FR.conds64(sd, torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)))
    full = (conds, torch.from_numpy(fx["text"]), torch.from_numpy(fx["text_lens"]), torch.from_numpy(fx["codes"]), torch.from_numpy(fx["wav_lengths"]))
    return sd, FR.Model(sd, 2), conds, full, ragged_batch(conds, fx)


def ragged_rows(conds, fx):
    """The overfit set as the trainer's ragged batch: three utterances of 9 / 4 / 6 codes, each its own sequence."""
    return dict(conds=conds, text_rows=[torch.from_numpy(fx["text"][i, : int(fx["text_lens"][i])]) for i in range(3)],
                code_rows=[torch.from_numpy(fx["codes"][i, :n]) for i, n in enumerate((9, 4, 6))])


def ragged_batch(conds, fx):
    lens, n = [int(v) for v in fx["text_lens"]], (9, 4, 6)
    text = torch.full((3, max(lens)), FR.STOP_TEXT, dtype=torch.long)
    codes = torch.full((3, max(n)), FR.STOP_MEL, dtype=torch.long)
    for i in range(3):
        text[i, : lens[i]] = torch.from_numpy(fx["text"][i, : lens[i]])
        codes[i, : n[i]] = torch.from_numpy(fx["codes"][i, : n[i]])
    return conds, text, torch.tensor(lens), codes, torch.tensor(n) * 1024


def random_factors(sd, r=4, seed=5, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return {k: (A, torch.randn(B.shape, generator=g) * std) for k, (A, B) in FR.init_factors(sd, 2, r, seed).items()}


def test_restatement_meets_the_reference_fixture_at_b_zero(ref):
    sd, model, _, full, _ = ref
    fx = FR.fixture()
    with torch.no_grad():
        o = model.losses(*full, factors=FR.leaves(FR.init_factors(sd, 2, 4, 0), requires_grad=False), scaling=2.0)
    assert abs(float(o["loss_text"]) - float(fx["loss_text_64"])) < 1e-9 and abs(float(o["loss_mel"]) - float(fx["loss_mel_64"])) < 1e-9
    assert (o["mel_nll"].numpy() - fx["mel_nll"]).__abs__().max() < 1e-8 and (o["text_nll"].numpy() - fx["text_nll"]).__abs__().max() < 1e-8


def test_gradients_agree_with_central_differences(ref):
    sd, model, _, _, rb = ref
    f = random_factors(sd)
    _, g = FR.loss_and_grads(model, rb, f, 2.0, 0.1)

    def loss(ff):
        with torch.no_grad():
            o = model.losses(*rb, factors=FR.leaves(ff, requires_grad=False), scaling=2.0)
        return 0.1 * float(o["loss_text"]) + 0.9 * float(o["loss_mel"])
    h = 1e-5
    for key, j, idx in (("gpt.h.0.attn.c_attn", 0, (1, 7)), ("gpt.h.0.mlp.c_fc", 1, (300, 2)), ("gpt.h.1.attn.c_proj", 1, (5, 0)),
                        ("gpt.h.1.mlp.c_proj", 0, (3, 4000)), ("gpt.h.1.attn.c_attn", 1, (2000, 3))):
        up, dn = FR.leaves(f, requires_grad=False), FR.leaves(f, requires_grad=False)
        up[key][j][idx] += h
        dn[key][j][idx] -= h
        fd, an = (loss(up) - loss(dn)) / (2 * h), float(g[key][j][idx])
        print(key, "AB"[j], idx, fd, an)
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)) + 1e-9


def test_restated_optimizer_equals_torch_adamw_over_5_steps():
    g = torch.Generator().manual_seed(1)
    A, B = torch.randn(4, 33, generator=g).double(), torch.randn(17, 4, generator=g).double()
    grads = [(torch.randn(4, 33, generator=g).double(), torch.randn(17, 4, generator=g).double()) for _ in range(5)]
    pa, pb = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
    opt = torch.optim.AdamW([dict(params=[pa], lr=1e-3, weight_decay=0.01), dict(params=[pb], lr=2e-3, weight_decay=0.01)],
                            betas=(0.9, 0.999), eps=1e-8)

    tr = FR.Trainer(None, {"k": (A, B)}, 1.0, lr=1e-3, ratio=2.0, wd=0.01, max_norm=None, total_steps=10 ** 9, warmup_ratio=0.0)
    tr.f = {"k": (A.clone(), B.clone())}
    for ga, gb in grads:
        pa.grad, pb.grad = ga.clone(), gb.clone()
        opt.step()
        assert abs(tr.apply({"k": (ga, gb)})["lr"] - 1e-3) < 1e-12          # (a cosine over 1e9 steps: flat here)
        assert (tr.f["k"][0] - pa.detach()).abs().max() < 1e-12 and (tr.f["k"][1] - pb.detach()).abs().max() < 1e-12
    # and one update of adamw64, the kernel's reference, is that same update
    p2, m1, v1, *_ = FR.adamw64(A, grads[0][0], torch.zeros_like(A), torch.zeros_like(A), 1e-3, 0.01, 1)
    q = A.clone().requires_grad_(True)
    o2 = torch.optim.AdamW([q], lr=1e-3, weight_decay=0.01)
    q.grad = grads[0][0].clone()
    o2.step()
    assert (p2 - q.detach()).abs().max() < 1e-14


def test_trainer_step_is_torch_adamw_with_clipping(ref):
    """Trainer.step itself (its gradients, clipping, groups and schedule) against torch.optim.AdamW + clip_grad_norm_ + LambdaLR."""
    sd, model, _, _, rb = ref
    f = random_factors(sd)
    tr = FR.Trainer(model, f, 2.0, lr=1e-3, total_steps=8, warmup_ratio=0.25)
    fl = FR.leaves(f)
    A_params, B_params = [ab[0] for ab in fl.values()], [ab[1] for ab in fl.values()]
    opt = torch.optim.AdamW([dict(params=A_params, lr=1e-3, weight_decay=0.01), dict(params=B_params, lr=2e-3, weight_decay=0.01)])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: FR.cosine_with_warmup(s, 2, 8))
    for _ in range(3):
        rep = tr.step(rb)
        opt.zero_grad()
        with torch.enable_grad():
            o = model.losses(*rb, factors=fl, scaling=2.0)
            (0.1 * o["loss_text"] + 0.9 * o["loss_mel"]).backward()
        norm = torch.nn.utils.clip_grad_norm_(A_params + B_params, 1.0)
        opt.step()
        sched.step()
        assert abs(float(norm) - rep["grad_norm"]) <= 1e-9 * float(norm)
    for k in fl:
        for j in range(2):
            assert (fl[k][j].detach() - tr.f[k][j]).abs().max() <= 1e-12


def test_schedule():
    from indextts.gpt.fit import cosine_with_warmup
    try:
        from transformers import get_cosine_schedule_with_warmup
    except Exception:                                  # not installed: the formula alone
        get_cosine_schedule_with_warmup = None
    for warm, total in ((0, 10), (3, 24), (10, 100), (5, 5)):
        want = None
        if get_cosine_schedule_with_warmup is not None:
            p = torch.nn.Parameter(torch.zeros(1))
            opt = torch.optim.SGD([p], lr=1.0)
            sch = get_cosine_schedule_with_warmup(opt, warm, total)
            want = []
            for _ in range(total + 2):
                want.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
        for s in range(total + 2):
            f = s / max(1, warm) if s < warm else max(0.0, 0.5 * (1 + math.cos(math.pi * (s - warm) / max(1, total - warm))))
            assert abs(cosine_with_warmup(s, warm, total) - f) < 1e-15 and abs(FR.cosine_with_warmup(s, warm, total) - f) < 1e-15
            if want is not None:
                assert abs(want[s] - f) < 1e-12


def test_ragged_batch_is_each_utterance_alone(ref):
    """The ragged form's losses are the position-weighted means of the utterances' own; the longest utterance's positions are those
    of the padded batch (nothing in front of them is padding there)."""
    sd, model, conds, _, rb = ref
    rows = ragged_rows(conds, FR.fixture())
    with torch.no_grad():
        o, padded = FR.batch_losses(model, rows), model.losses(*rb)
    assert [len(x) for x in o["mel_nll"]] == [11, 6, 8] and [len(x) for x in o["text_nll"]] == [14, 11, 8]
    assert abs(float(o["loss_mel"]) - float(torch.cat(o["mel_nll"]).sum()) / 25) < 1e-12
    assert (o["mel_nll"][0] - padded["mel_nll"][0]).abs().max() < 1e-9 and (o["mel_nll"][1][:5] - padded["mel_nll"][1][:5]).abs().max() > 1e-6


def test_b_zero_start(ref):
    sd, model, _, _, rb = ref
    _, g = FR.loss_and_grads(model, rb, FR.init_factors(sd, 2, 4, 0), 2.0, 0.1)
    for key, (dA, dB) in g.items():
        assert not dA.any(), key
        assert dB.abs().max() > 0, key


def test_initialisation_is_pefts_and_the_trainers():
    from indextts.gpt.fit import init_factors
    sd = gpt_state()
    ref_f = FR.init_factors(sd, 2, 4, 7)
    gen = torch.Generator().manual_seed(7)
    for i in range(2):
        for name in FR.TARGETS:
            K, N = sd[f"gpt.h.{i}.{name}.weight"].shape
            A, Bt = init_factors(K, N, 4, gen)
            assert torch.equal(A, ref_f[f"gpt.h.{i}.{name}"][0]) and not Bt.any() and Bt.shape == (4, N)
            assert A.abs().max() <= 1 / math.sqrt(K) and A.abs().max() > 0.9 / math.sqrt(K)
    layer = torch.nn.Linear(1280, 4, bias=False)               # peft: kaiming_uniform_(lora_A.weight, a=sqrt(5))
    torch.nn.init.kaiming_uniform_(layer.weight, a=math.sqrt(5))
    assert layer.weight.abs().max() <= 1 / math.sqrt(1280)


def test_overfit_budget_halves_loss_mel_in_float64(ref):
    """The condition that gives the device's overfit test its meaning: the float64 trajectory alone, under FR.OVERFIT, brings
    loss_mel under half its start, with room (under 0.35 of it)."""
    sd, model, conds, _, _ = ref
    rb = ragged_rows(conds, FR.fixture())
    c = FR.OVERFIT
    tr = FR.Trainer(model, FR.init_factors(sd, 2, c["rank"], 0), c["alpha"] / c["rank"], lr=c["lr"], wd=c["weight_decay"],
                    text_weight=c["text_weight"], max_norm=c["max_grad_norm"], total_steps=c["steps"], warmup_ratio=c["warmup_ratio"])
    first = tr.step(rb)["loss_mel"]
    for _ in range(c["steps"] - 1):
        tr.step(rb)
    with torch.no_grad():
        last = float(FR.batch_losses(model, rb, factors=tr.f, scaling=tr.scaling)["loss_mel"])
    print(f"float64 overfit: loss_mel {first:.4f} -> {last:.4f}")
    assert last < 0.35 * first


# ------------------------------------------------------------------------------------------------------------------ host checks
class FakeEngine:
    weight_dtype = kv_dtype = None
    lora = False


def test_host_refusals():
    from indextts.gpt.fit import FitConfig, check_engine, check_rows, plan_batches
    for bad in (0, 65, 4.0):
        with pytest.raises(ValueError, match="rank"):
            FitConfig(rank=bad).check()
    for bad in ((), ("attn.c_attn", "attn.q"), ("mlp.c_fc", "mlp.c_fc")):
        with pytest.raises(ValueError, match="targets"):
            FitConfig(targets=bad).check()
    with pytest.raises(ValueError, match="dropout"):
        FitConfig(dropout=1.0).check()
    with pytest.raises(ValueError, match="text_weight"):
        FitConfig(text_weight=1.5).check()
    assert FitConfig(rank=64, targets=("mlp.c_fc",)).check().rank == 64
    d = FitConfig()
    assert (d.rank, d.alpha, d.text_weight, d.loraplus_lr_ratio, d.dropout, d.lr, d.weight_decay) == (4, 8.0, 0.1, 2.0, 0.2, 5e-6, 0.01)
    e = FakeEngine()
    check_engine(e)
    e.weight_dtype = "fp8"
    with pytest.raises(ValueError, match="FP8"):
        check_engine(e)
    e.weight_dtype, e.kv_dtype = None, "fp8"
    with pytest.raises(NotImplementedError, match="FP8 KV"):
        check_engine(e)
    e.kv_dtype, e.lora = None, True
    with pytest.raises(ValueError, match="attach_lora"):
        check_engine(e)
    t, c = [torch.zeros(5), torch.zeros(3)], [torch.zeros(9), torch.zeros(4)]
    with pytest.raises(ValueError, match="1 code rows for 2 texts"):
        check_rows(t, c[:1], 100)
    with pytest.raises(ValueError, match="no utterance"):
        check_rows([], [], 100)
    with pytest.raises(ValueError, match="no text tokens or no codes"):
        check_rows(t, [c[0], torch.zeros(0)], 100)
    with pytest.raises(ValueError, match="too small for the longest utterance \\(50 rows\\)"):
        check_rows(t, c, 49, n_cond=32)
    assert check_rows(t, c, 50, n_cond=32) == [50, 43]
    assert plan_batches([50, 43, 10, 60], 100) == [[0, 1], [2], [3]] and plan_batches([50, 43], 50) == [[0], [1]]


def test_cli_parsing():
    from indextts.cli import fit_voice_parser
    a = fit_voice_parser().parse_args(["--fit-voice", "d", "-v", "p.wav", "--out", "v.pt"])
    assert (a.fit_voice, a.voice, a.out, a.rank, a.alpha, a.steps, a.lr, a.batch_rows, a.text_weight, a.dropout, a.seed, a.save_merged) == \
        ("d", "p.wav", "v.pt", 4, 8.0, 100, 5e-6, 4096, 0.1, 0.2, 0, None)
    a = fit_voice_parser().parse_args("--fit-voice d -v p --out v --rank 8 --alpha 16 --steps 7 --lr 1e-4 --batch-rows 512 --text-weight 0.2 "
                                      "--dropout 0 --seed 3 --save-merged m.pth".split())
    assert (a.rank, a.alpha, a.steps, a.lr, a.batch_rows, a.text_weight, a.dropout, a.seed, a.save_merged) == (8, 16.0, 7, 1e-4, 512, 0.2, 0.0, 3, "m.pth")
    with pytest.raises(SystemExit):
        fit_voice_parser().parse_args(["--fit-voice", "d"])


def test_merged_state_dict_round_trips_keys_and_dtypes(tmp_path):
    from indextts.gpt.fit import merged_state_dict
    sd = {k: (v.to(torch.float16) if v.is_floating_point() else v) for k, v in gpt_state().items()}
    f = random_factors(sd, r=4)
    merged = merged_state_dict(sd, f, 2.0, 2)
    path = tmp_path / "gpt_finetuned.pth"
    torch.save(merged, path)
    back = torch.load(path, weights_only=True)
    assert list(back) == list(sd) and all(back[k].dtype == sd[k].dtype and back[k].shape == sd[k].shape for k in sd)
    for k in sd:
        if k[: -len(".weight")] in f:
            A, B = f[k[: -len(".weight")]]
            want = (sd[k].double() + 2.0 * (B.double() @ A.double()).t()).to(torch.float16)
            assert torch.equal(back[k], want) and not torch.equal(back[k], sd[k])
        else:
            assert torch.equal(back[k], sd[k])
    with pytest.raises(ValueError, match="unknown adapter targets"):
        merged_state_dict(sd, {"gpt.h.9.mlp.c_fc": f["gpt.h.0.mlp.c_fc"]}, 2.0, 2)
