"""The float64 references of tests/frontend_refs.py are right, and the negative controls of tests/test_frontend_kernels_gpu.py
discriminate -- both shown without a GPU.

Part 1 holds every reference, with its intermediate roundings switched off, to torch's own float64 operators (F.conv2d, F.glu +
F.conv1d(groups=C) + F.layer_norm + F.silu, F.pad(mode="reflect") + F.conv1d(dilation=), torch.softmax, F.gelu, F.normalize)
at about 1e-12 relative, on operands of its own seeds.  Part 2 applies each control to the reference alone, on the very operands
of the GPU case that runs the control -- the generators of frontend_refs derive their seeds from the case, and both tests call
them with the case alone: the controlled reference must differ from the true one by more than the bound the GPU test asserts,
somewhere."""
import math

import pytest
import torch
import torch.nn.functional as F

import frontend_refs as R

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
TOL = 1e-12


def close(a, b, what):
    err = (a - b).abs().max().item()
    lim = TOL * max(1.0, b.abs().max().item())
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def moved(what, ref, bad, bound, valid=None):
    """A control discriminates when it moves some element of the reference by more than that element's bound."""
    r = (bad - ref).abs() / bound
    if valid is not None:
        r = torch.where(valid, r, torch.zeros_like(r))
    assert r.max().item() > 1.0, f"{what}: the control moves the reference by {r.max().item():.3f} of the bound at most"


# ------------------------------------------------------------------------------------------------------ part 1
@pytest.mark.parametrize("T,Fq,C", [(7, 20, 64), (3, 5, 8), (4, 145, 8)])
def test_subsample_conv_ref_is_conv2d(T, Fq, C):
    mel, w, b = R.subsample_inputs(T, Fq, C, seed=1)
    ref, S = R.subsample_conv_ref(mel, w, b)
    t = F.relu(F.conv2d(mel.double()[None, None], w.double().view(C, 1, 3, 3), b.double(), stride=2))[0]
    close(ref, t.permute(1, 0, 2).reshape(ref.shape), "subsample_conv")
    assert (S >= ref.abs() - 1e-9).all()


@pytest.mark.parametrize("Tk", [1, 32, 33, 129, 161])
@pytest.mark.parametrize("rel", [False, True])
def test_mha_small_walk_is_softmax_attention(Tk, rel):
    q, k, v, pos, bu, bv = R.mha_inputs(19, Tk, 2, rel, BF16, seed=3)
    ref, _, info = R.mha_small_ref(q, k, v, 0.125, pos, bu, bv, exact=True)
    close(ref, R.mha_oneshot(q, k, v, 0.125, pos, bu, bv), f"mha walk Tk={Tk}")
    assert info["P_j"].shape == (2, 19, Tk) and not info["near"].any()
    # with the roundings on, the walk stays within its own bound of the exact result's neighbourhood (the bound is not vacuous)
    r2, E, _ = R.mha_small_ref(q, k, v, 0.125, pos, bu, bv)
    assert torch.isfinite(r2).all() and (E > 0).all() and (E < 0.05).all()


GLU = [(1, 128, 31, 0), (9, 128, 15, 0), (17, 256, 7, None), (33, 512, 15, None), (5, 2048, 15, 0), (5, 2048, 15, 1), (5, 2048, 15, 2)]


@pytest.mark.parametrize("T,C,taps,cls", GLU, ids=["%d-%d-%d" % c[:3] + ("-class%d" % c[3] if c[3] else "") for c in GLU])
def test_glu_dwconv_ln_silu_ref_is_torch(T, C, taps, cls):
    x, w, b, lw, lb = R.glu_inputs(T, C, taps, BF16, cls, seed=5)
    ref, bound = R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, dtype=BF16)
    g = F.glu(x.double().t()[None], dim=1)
    c = F.conv1d(g, w.double()[:, None, :], b.double(), padding=(taps - 1) // 2, groups=C)[0].t()
    close(ref, F.silu(F.layer_norm(c, (C,), lw.double(), lb.double(), 1e-5)), "glu_dwconv_ln_silu")
    assert (bound > 0).all()
    quiet = torch.arange(C) != 5                                        # the outlier channel aside
    ratio = c[:, quiet].mean(1).abs() / c[:, quiet].std(1)
    if cls is None:  # the rows' |mean| / sigma classes exist (glu_inputs)
        assert ratio.min() < 1.0 and ratio.max() > 64.0 and ((ratio > 4) & (ratio < 16)).any(), ratio
    else:            # every row is of the one class
        lo, hi = ((0.0, 1.0), (4.0, 16.0), (64.0, math.inf))[cls]
        assert (ratio > lo).all() and (ratio < hi).all(), ratio
    r = R.glu_outlier_row(T, cls)
    out = (c[r, 5] - c[r, quiet].mean()) / c[r, quiet].std()
    assert 40.0 < out < 90.0, out                                      # one channel of one row's conv output stands 60 sigma out
    if T > 1:
        others = ((c[:, 5] - c[:, quiet].mean(1)) / c[:, quiet].std(1))[torch.arange(T) != r]
        assert (others.abs() < 40.0).all(), others


def test_rows_ref_is_torch():
    M, D = 5, 64
    x, slab, bias = R.rnd(M, D, seed=7).float(), R.rnd(9, M, D, seed=8).float(), R.rnd(D, seed=9).float()
    w, b = (1 + 0.1 * R.rnd(D, seed=10)).float(), R.rnd(D, seed=11).float()
    v = x.double() + bias.double() + slab.double().sum(0)
    close(R.rows_ref(M, D, x, slab, bias)[0], v, "rows norm 0")
    close(R.rows_ref(M, D, x, slab, bias, 1, w, b)[0], F.layer_norm(v, (D,), w.double(), b.double(), 1e-5), "rows norm 1")
    close(R.rows_ref(M, D, x, slab, bias, 2, w)[0], F.normalize(v, dim=-1) * math.sqrt(D) * w.double(), "rows norm 2")
    z = R.rows_ref(1, D, torch.zeros(1, D), None, None, 2, w)
    assert (z[0] == 0).all() and torch.isfinite(z[1]).all()


def test_geglu_ref_is_gelu():
    h = R.geglu_inputs(17, 96, F16, seed=12)
    close(R.geglu_ref(h)[0], F.gelu(h[:, 96:].double()) * h[:, :96].double(), "geglu")
    g = h[:, 96:].double()
    assert (g == 0).any() and (g < -5.5).any() and (g > 5.5).any()


@pytest.mark.parametrize("T,Fq,taps,dil,Kp", [(3, 5, 5, 1, 32), (9, 8, 7, 2, 64), (10, 12, 3, 3, 64)])
def test_im2col_ref_is_reflect_pad(T, Fq, taps, dil, Kp):
    x = R.rnd(T, Fq, seed=13).float()
    pad = (taps - 1) // 2 * dil
    xp = F.pad(x.double().t()[None], (pad, pad), mode="reflect")[0].t()
    want = torch.cat([xp[j * dil:j * dil + T] for j in range(taps)], 1)
    got = R.im2col_reflect_ref(x, taps, dil, Kp)
    assert torch.equal(got[:, :taps * Fq], want) and (got[:, taps * Fq:] == 0).all()


@pytest.mark.parametrize("T,dil,s,first", [(2, 1, 1, True), (5, 4, 2, False), (17, 2, 7, False)])
def test_res2_step_ref_is_conv1d(T, dil, s, first):
    y1, cat = R.rnd(T, 512, seed=14).to(BF16), R.rnd(T, 512, seed=15).to(BF16)
    w = R.rnd(64, 64, 3, seed=16, scale=0.08).to(BF16)
    b, sc, sh = R.rnd(64, seed=17).float(), (1 + 0.1 * R.rnd(64, seed=18)).float(), R.rnd(64, seed=19).float()
    ref, _ = R.res2_step_ref(y1, cat, w, b, sc, sh, s, dil, first, BF16, exact=True)
    inp = y1[:, 64 * s:64 * s + 64].double() + (0 if first else cat[:, 64 * s - 64:64 * s].double())
    z = F.conv1d(F.pad(inp.t()[None], (dil, dil), mode="reflect"), w.double(), b.double(), dilation=dil)[0].t()
    close(ref, F.relu(z) * sc.double() + sh.double(), "res2_step")


def test_se_gate_scale_resid_col_stats_refs_are_torch():
    T, C, H = 37, 64, 16
    y, w1, b1, w2, b2 = R.se_inputs(T, C, H, F16, seed=20)
    g, _ = R.se_gate_ref(y, w1, b1, w2, b2, 3)
    close(g, torch.sigmoid(F.linear(F.relu(F.linear(y.double().mean(0), w1.double(), b1.double())), w2.double(), b2.double())), "se_gate")
    res = R.rnd(T, C, seed=21).to(F16)
    close(R.scale_resid_ref(y, res, g.float(), F16)[0], g.float().double() * y.double() + res.double(), "scale_resid")
    x, logit, sc, sh = R.col_stats_inputs(T, C, F16, seed=22)
    xd = x.double()
    m = xd.mean(0)
    close(R.col_stats_ref(x, 3, F16)[0], torch.cat([m, ((xd - m) ** 2).mean(0).clamp(1e-12).sqrt()]), "col_stats plain")
    a = torch.softmax(logit.double(), 0)
    m = (a * xd).sum(0)
    want = torch.cat([m, (a * (xd - m) ** 2).sum(0).clamp(1e-12).sqrt()]) * sc.double() + sh.double()
    close(R.col_stats_ref(x, 3, F16, logit, sc, sh)[0], want, "col_stats weighted")
    assert R.col_stats_ref(x, 3, F16)[0][C + 3].item() == 1e-6                     # the constant channel sits on the clamp


# ------------------------------------------------------------------------------------------------------ part 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_subsample_conv(dtype):
    mel, w, b = R.subsample_inputs(7, 20, 64)
    ref, S = R.subsample_conv_ref(mel, w, b)
    bound = R.subsample_conv_bound(ref, S, dtype)
    moved("window shifted", ref, R.subsample_conv_ref(mel, w, b, row_shift=1)[0], bound)
    bz = b.clone()
    bz[-1] = 0
    moved("last bias omitted", ref, R.subsample_conv_ref(mel, w, bz)[0], bound)
    moved("ReLU dropped", ref, R.subsample_conv_ref(mel, w, b, relu=False)[0], bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_mha_small(dtype):
    args = R.mha_inputs(16, 32, 1, True, dtype)
    ref, E, _ = R.mha_small_ref(*args[:3], 0.125, *args[3:])
    bound = R.mha_small_bound(ref, E, dtype)
    for name, bad in R.mha_controls(*args):
        moved(name, ref, bad, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_glu_dwconv_ln_silu(dtype):
    # the first case (T = 1) has no second row for a padding control: the controls run at the first case with T > (taps - 1) / 2
    x, w, b, lw, lb = R.glu_inputs(9, 128, 15, dtype, 0)
    ref, bound = R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, dtype=dtype)
    moved("first tap dropped", ref, R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, drop_tap=0)[0], bound)
    moved("padding replicated", ref, R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, replicate=True)[0], bound)
    moved("halves exchanged", ref, R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, swap_halves=True)[0], bound)
    moved("variance over C - 1", ref, R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, var_div=127)[0], bound)


def test_controls_rows():
    M, D = 37, 1280
    x, slab, bias, _, _ = R.rows_inputs(M, D, 9, 0)
    ref, bound = R.rows_ref(M, D, x, slab, bias)
    moved("slab 8 dropped", ref, R.rows_ref(M, D, x, slab, bias, drop_slab=8)[0], bound)
    moved("bias twice", ref, R.rows_ref(M, D, x, slab, bias, bias_twice=True)[0], bound)
    x, slab, bias, w, b = R.rows_inputs(M, D, 9, 1)
    ref, bound = R.rows_ref(M, D, x, slab, bias, 1, w, b)
    moved("LayerNorm without the mean", ref, R.rows_ref(M, D, x, slab, bias, 1, w, b, no_mean=True)[0], bound)
    x, slab, bias, w, _ = R.rows_inputs(M, D, 9, 2)
    ref, bound = R.rows_ref(M, D, x, slab, bias, 2, w)
    moved("sqrt(D) dropped", ref, R.rows_ref(M, D, x, slab, bias, 2, w, no_sqrt_d=True)[0], bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_geglu(dtype):
    h = R.geglu_inputs(1, 32, dtype)
    ref, bound = R.geglu_ref(h, dtype)
    moved("halves exchanged", ref, R.geglu_ref(h, swap_halves=True)[0], bound)
    cut = ref.clone()
    cut[:, -4:] = R.SENT
    moved("last 4-column group missing", ref, cut, bound)


def test_controls_im2col_reflect():
    x = R.im2col_inputs(3, 5)
    ref = R.im2col_reflect_ref(x, 5, 1, 32)
    for mode in ("replicate", "symmetric"):
        assert not torch.equal(R.im2col_reflect_ref(x, 5, 1, 32, mode).to(BF16), ref.to(BF16)), mode


@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_res2_step(dtype):
    for T, dil, s, first in ((17, 2, 7, False), (45, 3, 1, True)):        # the two GPU cases that run the controls
        a = (*R.res2_inputs(T, dtype), s, dil, first, dtype)
        ref, bound = R.res2_step_ref(*a)
        moved("replicate padding", ref, R.res2_step_ref(*a, mode="replicate")[0], bound)
        moved("taps reversed", ref, R.res2_step_ref(*a, reverse_taps=True)[0], bound)
        moved("BatchNorm shift omitted", ref, R.res2_step_ref(*a, no_shift=True)[0], bound)
        if not first:
            moved("previous chunk not added", ref, R.res2_step_ref(*a, add_prev=False)[0], bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_controls_se_gate_scale_resid_col_stats(dtype):
    T, C, H = 1, 64, 16
    y, w1, b1, w2, b2 = R.se_inputs(T, C, H, dtype)
    ref, bound = R.se_gate_ref(y, w1, b1, w2, b2, 1)
    moved("mean over the padded rows", ref, R.se_gate_ref(y, w1, b1, w2, b2, 1, rows=R.padded(y, 1))[0], bound)
    moved("b1 omitted", ref, R.se_gate_ref(y, w1, b1, w2, b2, 1, no_b1=True)[0], bound)
    moved("ReLU dropped", ref, R.se_gate_ref(y, w1, b1, w2, b2, 1, relu=False)[0], bound)
    yy, res, gate = R.scale_resid_inputs(1, 32, dtype)
    yy, res = R.padded(yy, 1), R.padded(res, 1, 500.0)                 # the kernel maps the padding rows too
    ref, bound = R.scale_resid_ref(yy, res, gate, dtype)
    moved("gate shifted by 8 channels", ref, R.scale_resid_ref(yy, res, gate, dtype, gate_shift=8)[0], bound)
    T, C = 17, 64
    x, logit, sc, sh = R.col_stats_inputs(T, C, dtype)
    ref, bound = R.col_stats_ref(x, 2, dtype)
    moved("statistics over the padded rows", ref, R.col_stats_ref(R.padded(x, 2), 2, dtype)[0], bound)
    moved("variance over T - 1", ref, R.col_stats_ref(x, 2, dtype, var_div_t1=True)[0], bound)
    ref, bound = R.col_stats_ref(x, 2, dtype, logit, sc, sh)
    moved("uniform weights", ref, R.col_stats_ref(x, 2, dtype, logit, sc, sh, uniform=True)[0], bound)
    moved("shift[C + c] from shift[c]", ref, R.col_stats_ref(x, 2, dtype, logit, sc, sh, shift_low=True)[0], bound)
