"""The float64 reference of tests/plain_gemm_refs.py is right, its bounds discriminate at the shapes the GPU cases use, and the
derived fp32 gelu term covers the kernel's chain -- all shown without a GPU.

Part 1 holds the reference of every case of tests/test_plain_gemm_kernels_gpu.py, on that case's own operands (the generator derives
its seeds from the case), to torch's own float64 operators (F.linear, F.gelu(approximate="tanh"), slices cut here from the header's
rule) at 1e-12 relative.  Part 2 lets the reference itself, rounded to the output type, stand in for the kernel's output: it stays
within the bound, and against every control of the case it leaves the bound -- the very comparison the GPU test makes.  Part 3
evaluates the kernel's gelu_new chain in numpy float32 on the fp32 gelu cases' pre-activations: twice its worst error fits under the
derived term G32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plain_forms as forms
import plain_gemm_refs as R
from fp64_check import excess

CUS = 256
CASES = [c.at(CUS) for c in R.CASES]
RUNS = [(c, dt) for c in CASES for dt in c.dts]
ids = lambda r: f"{R.TAG[r[1]]}-{r[0]}".replace(" ", "_")  # noqa: E731


@pytest.mark.parametrize("run", [r for r in RUNS if r[1] != R.F16], ids=ids)
def test_reference_is_the_torch_float64_formula(run):
    c, dtype = run
    o = R.operands(c, dtype)
    ref, S, _ = R.plain_ref(c, dtype, o)
    x, w = o["x"].double(), o["w"].double()
    if c.ks > 1:
        KS = 16 if dtype == R.F32 else 32
        KT = c.K // KS
        want = torch.stack([x[0, :, (s * KT) // c.ks * KS:((s + 1) * KT) // c.ks * KS] @ w[(s * KT) // c.ks * KS:((s + 1) * KT) // c.ks * KS]
                            for s in range(c.ks)])
    else:
        b = None if o["bias"] is None else o["bias"].double()
        want = F.linear(x, w.t(), b)
        if c.bias2:
            want = want + o["bias2"].double()[:, None]
        if c.act:
            want = F.gelu(want, approximate="tanh")
        if c.resid:
            want = want + o["resid"].double()
        want = want * float(np.float32(c.scale))
        if c.acc:
            want = want + o["y_prev"].double()
    assert ref.shape == want.shape == (max(c.B, c.ks), c.M, c.N)
    err, lim = (ref - want).abs().max().item(), 1e-12 * max(1.0, want.abs().max().item())
    assert err <= lim, f"{c}: {err:.3e} > {lim:.3e}"
    assert (S >= ref.abs() * (1 - 1e-12)).all() or c.act, f"{c}: S is not a magnitude sum"


@pytest.mark.parametrize("run", [r for r in RUNS if r[0].ctl], ids=ids)
def test_bounds_discriminate_every_control(run):
    c, dtype = run
    o = R.operands(c, dtype)
    ref, S, pre = R.plain_ref(c, dtype, o)
    bound = R.bound(c, dtype, ref, S, pre)
    stand_in = ref.to(c.out_dtype(dtype))
    ratio, _ = excess(stand_in, ref, bound)
    assert ratio <= 0.5 + 1e-9 if c.out_dtype(dtype) != R.F32 else ratio <= 0.125, f"{c}: the rounded reference sits at {ratio:.3f} of its own bound"
    for name in c.ctl:
        wrong = R.plain_ref(c, dtype, o, ctl=name)[0]
        r, (idx, *_) = excess(stand_in, wrong, bound)
        assert r > 1.0, f"{c} {R.TAG[dtype]}: control '{R.CONTROLS[name]}' stays within the bound ({r:.3f} at {idx})"


def test_every_control_and_family_is_used():
    used = {n for c in CASES for n in c.ctl}
    assert used == set(R.CONTROLS), set(R.CONTROLS) - used
    for fam in ("m-edge", "k-edge", "split-k", "epilogue", "wide", "n64"):
        first = next(c for c in CASES if c.fam == fam)
        assert first.ctl, f"the first case of {fam} carries no control"


def test_cases_reach_the_forms_and_paths_they_are_there_for():
    """The case list against the dispatch rules (plain_forms): every reachable form, both L2 patch heights, the slice shapes."""
    got = {forms.form(R.TAG[dt], c.B, c.M, c.N, c.K, c.ks, CUS) for c, dt in RUNS}
    assert got == forms.REACHABLE, forms.REACHABLE ^ got
    order = [c for c in CASES if c.fam == "tile-order"]
    assert {forms.l2_patch_gm(128, c.K // 32) for c in order} == {4, 8}
    for c in order:
        gm, mb = forms.l2_patch_gm(128, c.K // 32), (c.M + 127) // 128
        assert mb > gm and mb % gm != 0 and (mb * (c.N // 128)) % 8 != 0       # a full and a partial patch; a grid that is no multiple of 8
    wide = [c for c in CASES if c.fam == "wide" and c.M > 300]
    assert wide and all(c.M == 103 * 128 - 57 for c in wide)                     # 103 m-blocks on a 256-CU part
    assert forms.slice_ksteps(40, 3, 1) == (13, 26) and forms.slice_ksteps(40, 3, 2) == (26, 40)    # 13, 13, 14 steps; kt0 = 13, 26
    assert {(c.K, c.ks) for c in CASES if c.fam == "split-k"} == {(1280, 2), (1280, 3), (128, 4), (2048, 64), (5120, 3)}
    assert all(not (c.K <= 64 and c.N <= 64) for c in CASES)


def test_gelu_f32_term_holds_twice_the_emulation():
    """G32 is derived (module docstring of plain_gemm_refs); here the kernel's chain, step by step in numpy float32, on the fp32 gelu
    cases' own pre-activations and on a grid over [-12, 12]: twice its worst error fits under G32, and the recorded figure is this one."""
    worst, at = 0.0, 0.0
    pres = [R.plain_ref(c, R.F32, R.operands(c, R.F32))[2].flatten() for c in CASES if c.act and R.F32 in c.dts]
    assert len(pres) >= 8
    for pre in pres + [torch.linspace(-12.0, 12.0, 200001, dtype=torch.float64)]:
        p32 = pre.numpy().astype(np.float32)
        p = torch.from_numpy(p32.astype(np.float64))
        err = (torch.from_numpy(R.gelu_chain_f32(p32).astype(np.float64)) - R.gelu_new(p)).abs()
        r = err / R.gelu_f32_term(p)
        i = int(torch.argmax(r))
        if r[i].item() > worst:
            worst, at = r[i].item(), p[i].item()
    print(f"fp64 | measure | gelu_new fp32 chain emulated in numpy float32: worst err / G32 (at p = {at:.3f}) | {worst:.3f}")
    assert 2.0 * worst <= 1.0, (worst, at)
    assert abs(worst - R.EMU_G32) < 0.01, f"plain_gemm_refs.EMU_G32 records {R.EMU_G32}, measured {worst:.3f}"
