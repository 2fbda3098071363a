"""The float64 references of tests/vocoder_refs.py are right, their fp32 bounds admit an honest fp32 evaluation and discriminate -- all
shown without a GPU.

Part 1 holds every reference to torch's own float64 operators: `conv_ref` to F.conv1d (explicit zero padding, dilation, ragged lengths
as zeroed rows), the up-sampler's slice of it to F.conv_transpose1d, `act_ref` to oracle.bigvgan_ref.activation1d, `tanh_ref` to
torch.tanh, all below 1e-12.  Part 2 lets plain torch fp32 on the CPU stand in for the kernel on the operands of the GPU file's cases
(shifted fp32 matmuls, the oracle's activation run in fp32, torch.tanh in fp32): it passes `check` under every fp32 bound, and every
negative control fails `must_fail` against it, the very comparison tests/test_vocoder_fp32_kernels_gpu.py makes.  Part 3 fixes the
control magnitudes: TAP32[family] is the smallest power of two at which the perturbed float64 reference itself leaves the bound on the
first case of that family -- computed here in float64 alone.  Part 4 holds the case lists against what they are there for: the dispatch
rule reaches every form of REACHABLE_F32_CONV, and the float64 PCM reference alone stays under the 1 % cap for every tanh_pcm case."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_refs as R
from fp64_check import check, excess, must_fail

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def fir():
    from indextts.BigVGAN.models import kaiser_sinc_filter
    f = kaiser_sinc_filter()
    return f, f


def close(what, ref, want, tol=1e-12):
    assert ref.shape == want.shape, what
    err = (ref - want).abs().max().item()
    assert err < tol * max(1.0, want.abs().max().item()), f"{what}: {err:.3e}"


def stand_in_conv(x, w, k, off0, d, T, bias, rk, vr=None):
    """The convolution and its epilogue in plain torch fp32."""
    B, Tin, _ = x.shape
    xs = x if vr is None else x * (torch.arange(Tin)[None, :] < vr.long()[:, None])[..., None]
    acc = torch.zeros(B, T, w.shape[2], dtype=F32)
    for j in range(k):
        s = off0 + j * d
        lo, hi = max(0, -s), min(T, Tin - s)
        if hi > lo:
            acc[:, lo:hi] += xs[:, lo + s:hi + s] @ w[j]
    acc = acc + bias
    if "bias2" in rk:
        acc = acc + rk["bias2"][:, None, :]
    if "resid" in rk:
        acc = acc + rk["resid"]
    acc = acc * torch.tensor(rk.get("scale", 1.0), dtype=F32)
    return acc + rk["yprev"] if "yprev" in rk else acc


def torch_conv64(x, w, k, off0, d, T, vr=None):
    """F.conv1d in float64 on explicitly zero-padded rows: what conv_ref computes without an epilogue."""
    xd = x.double()
    if vr is not None:
        xd = xd * (torch.arange(x.shape[1])[None, :] < vr.long()[:, None])[..., None]
    left, right = -off0, max(0, T + off0 + (k - 1) * d - x.shape[1])
    xp = F.pad(xd.transpose(1, 2), (left, right))
    return F.conv1d(xp, w.double().permute(2, 1, 0), dilation=d).transpose(1, 2)[:, :T]


# ----------------------------------------------------------------------------------------------------------- part 1
@pytest.mark.parametrize("C,N,k,d,T", [(24, 24, 7, 3, 257), (24, 1, 7, 1, 40), (40, 20, 11, 5, 70), (16, 32, 5, 16, 33), (8, 16, 2, 1, 9),
                                       (24, 40, 3, 32, 1), (96, 96, 3, 32, 130)])
def test_conv_reference_matches_torch_float64(C, N, k, d, T):
    for epi in R.EPI_MATRIX:
        x, w, bias, off0, rk = R.conv_case(F32, 2, T, C, N, k, d, epi, R.conv_seed(C, N, k, d, T))
        ref, mag = R.conv_ref(x, w, k, off0, d, T, bias=bias, **rk)
        want = torch_conv64(x, w, k, off0, d, T) + bias.double()
        if "bias2" in rk:
            want = want + rk["bias2"].double()[:, None, :]
        if "resid" in rk:
            want = want + rk["resid"].double()
        want = want * float(np.float32(rk.get("scale", 1.0)))
        if "yprev" in rk:
            want = want + rk["yprev"].double()
        close(f"conv {C}->{N} k={k} d={d} T={T} {epi}", ref, want)
        assert (mag >= ref.abs() * (1 - 1e-12)).all()
    vr = torch.tensor([0, T], dtype=torch.int32) if T < 3 else torch.tensor([1, T - 2], dtype=torch.int32)
    x, w, bias, off0, rk = R.conv_case(F32, 2, T, C, N, k, d, "bias", 5)
    close("ragged", R.conv_ref(x, w, k, off0, d, T, bias=bias, vr=vr)[0], torch_conv64(x, w, k, off0, d, T, vr) + bias.double())


@pytest.mark.parametrize("case", R.UPS, ids=lambda c: "%d-%dto%d" % c[:3])
def test_upsampler_reference_matches_torch_float64(case):
    Tn, cin, c, k, u = case
    B, Tn = 2, min(Tn, 21)
    x, w, bias, b2 = R.ups_case(F32, B, Tn, cin, c, k, u, 5000 + cin, bias2=True)
    taps, off0, shift = R.convtr_taps(w, u)
    rows = Tn + 1 if taps.shape[0] == 2 else Tn
    acc, _ = R.conv_ref(x, taps, taps.shape[0], off0, 1, rows, bias=bias, bias2=b2)
    want = F.conv_transpose1d(x.double().transpose(1, 2), w.double(), bias[:c].double(), stride=u, padding=(k - u) // 2).transpose(1, 2)
    assert want.shape == (B, Tn * u, c)
    want = want + R.ups_slice(b2.double()[:, None, :].expand(B, rows, u * c), shift, B, Tn * u, c)
    close(f"upsampler {cin}->{c}", R.ups_slice(acc, shift, B, Tn * u, c), want)


def test_act_reference_matches_the_oracle(fir):
    """The explicit 12-tap form of act_ref is oracle.bigvgan_ref.activation1d (conv_transpose / conv1d form) in float64, at every
    length up to 13 and one past a tile, and each element of a ragged batch is the same as run alone."""
    from oracle.bigvgan_ref import activation1d
    up, dn = fir
    for T in list(range(1, 14)) + [77]:
        x, al, be = R.act_case(torch.float64, 2, T, 8, seed=T)
        ref, _, _ = R.act_ref(x, al, be, up, dn, False)
        o = activation1d(x.transpose(1, 2), al.double(), be.double(), np.asarray(up, np.float64), np.asarray(dn, np.float64))
        close(f"act T={T}", ref, o.transpose(1, 2))
    x, al, be = R.act_case(F32, 3, 20, 8, seed=3)
    lens = [20, 7, 0]
    ref, _, ok = R.act_ref(x, al, be, up, dn, False, lens)
    close("ragged act", ref[1, :7], R.act_ref(x[1:2, :7], al, be, up, dn, False)[0][0])
    assert ok.sum().item() == 27 and (ref[2] == 0).all()


def test_tanh_reference_matches_torch_float64():
    x = R.tanh_inputs(257, F32, R.TANH_SEED, True)
    v, wb = R.tanh_ref(x, True)
    assert torch.equal(v, torch.tanh(x.double())) and (wb > 0).all()
    v, wb = R.tanh_ref(x, False)
    assert torch.equal(v, x.double()) and (wb == 0).all()


# ----------------------------------------------------------------------------------------------------------- part 2
def conv_stand_in_and_controls(family, B, T, C, N, k, d, epi, vr=None, controls=True):
    x, w, bias, off0, rk = R.conv_case(F32, B, T, C, N, k, d, epi, R.conv_seed(C, N, k, d, T))
    ref, mag = R.conv_ref(x, w, k, off0, d, T, bias=bias, vr=vr, **rk)
    bound = R.conv_bound(ref, mag, F32)
    y = stand_in_conv(x, w, k, off0, d, T, bias, rk, vr)
    what = f"fp32 stand-in, {R.f32_conv_form(C, N, k)} B={B} T={T} C={C} N={N} k={k} d={d} {epi}"
    valid = None if vr is None else (torch.arange(T)[None, :] < vr.long()[:, None])[..., None]
    print(f"fp64 | stand-in | {what} | {check(what, y, ref, bound, valid):.3f}")
    if controls:
        ctl = R.conv_controls(x, w, k, off0, d, T, bias, rk, R.TAP32[family] if epi == "bias" else None, vr)
        assert len(ctl) == 3 + (vr is None) + (epi == "bias"), list(ctl)
        for text, r_bad in ctl.items():
            print(f"fp64 | control | {what}: {text} | {must_fail(what, text, y, r_bad, bound, valid):.3f}")


@pytest.mark.parametrize("family", sorted(R.FIRST_CONV))
def test_conv_stand_in_passes_and_every_control_fails(family):
    C, N, k, d = R.FIRST_CONV[family]
    T = R.row_tile(R.f32_conv_form(C, N, k)) + 1
    for epi in R.CONTROL_EPIS:
        conv_stand_in_and_controls(family, 3, T, C, N, k, d, epi)


def test_conv_stand_in_passes_every_form_and_epilogue():
    """Every (Cin, N) of the GPU file's list at its first (k, d), one row past the form's tile, every epilogue of EPI_MATRIX."""
    for C, N, kds in R.F32_CONV_CASES:
        k, d = kds[0]
        T = R.row_tile(R.f32_conv_form(C, N, k)) + 1
        for epi in R.EPI_MATRIX:
            conv_stand_in_and_controls(None, 2, T, C, N, k, d, epi, controls=False)


def test_ragged_conv_stand_in_and_controls():
    for i, (C, N, k, d) in enumerate(R.RAGGED_F32):
        lens = R.ragged_lens(R.row_tile(R.f32_conv_form(C, N, k)))
        vr = torch.tensor(lens, dtype=torch.int32)
        for epi in ("bias", "resid_acc_third"):
            conv_stand_in_and_controls("ragged", len(lens), R.RAGGED_T, C, N, k, d, epi, vr=vr, controls=(i == 0))


def ups_refs(x, w, bias, b2, u, B, Tn, c):
    taps, off0, shift = R.convtr_taps(w, u)
    rows = Tn + 1 if taps.shape[0] == 2 else Tn

    def ref_of(tp):
        acc, mag = R.conv_ref(x, tp, tp.shape[0], off0, 1, rows, bias=bias, bias2=b2)
        return R.ups_slice(acc, shift, B, Tn * u, c), R.ups_slice(mag, shift, B, Tn * u, c)
    return taps, off0, shift, rows, ref_of


@pytest.mark.parametrize("i", range(len(R.UPS)))
def test_upsampler_stand_in_and_control(i):
    Tn, cin, c, k, u = R.UPS[i]
    B = 3
    x, w, bias, b2 = R.ups_case(F32, B, Tn, cin, c, k, u, 5000 + cin, bias2=(cin >= 768))
    taps, off0, shift, rows, ref_of = ups_refs(x, w, bias, b2, u, B, Tn, c)
    ref, mag = ref_of(taps)
    bound = R.conv_bound(ref, mag, F32)
    y = F.conv_transpose1d(x.transpose(1, 2), w, bias[:c], stride=u, padding=(k - u) // 2).transpose(1, 2)
    if b2 is not None:
        y = y + R.ups_slice(b2[:, None, :].expand(B, rows, u * c), shift, B, Tn * u, c)
    what = f"fp32 stand-in, upsampler B={B} Tn={Tn} {cin}->{c} k={k} u={u}"
    print(f"fp64 | stand-in | {what} | {check(what, y, ref, bound):.3f}")
    if i == 0:
        eps = R.TAP32["upsampler"]
        must_fail(what, "one weight tap off", y, ref_of(R.perturbed_tap(taps, taps.shape[0] - 1, eps))[0], bound)
        must_fail(what, "x through fp16", y, R.ups_slice(R.conv_ref(R.x_through_fp16(x), taps, taps.shape[0], off0, 1, rows, bias=bias, bias2=b2)[0],
                                                        shift, B, Tn * u, c), bound)


def test_conv_pre_stand_in_and_control():
    p = R.CONV_PRE
    x, w, bias, off0, rk = R.conv_case(F32, p["B"], p["T"], p["C"], p["N"], p["k"], p["d"], "bias", 6000)
    rk = {"bias2": (R.rnd(p["B"], p["N"], seed=6003) * 0.1).float()}
    ref, mag = R.conv_ref(x, w, p["k"], off0, 1, p["T"], bias=bias, **rk)
    bound = R.conv_bound(ref, mag, F32)
    y = stand_in_conv(x, w, p["k"], off0, 1, p["T"], bias, rk)
    what = "fp32 stand-in, conv_pre 1280->1536 k=7 (Cin taps = 8960)"
    print(f"fp64 | stand-in | {what} | {check(what, y, ref, bound):.3f}")
    r_bad = R.conv_ref(x, R.perturbed_tap(w, 3, R.TAP32["conv_pre"]), p["k"], off0, 1, p["T"], bias=bias, **rk)[0]
    must_fail(what, "one weight tap off", y, r_bad, bound)
    must_fail(what, "x through fp16", y, R.conv_ref(R.x_through_fp16(x), w, p["k"], off0, 1, p["T"], bias=bias, **rk)[0], bound)


def stand_in_act(x, al, be, up, dn, lens=None):
    """oracle.bigvgan_ref.activation1d run in fp32, each element at its own length."""
    from oracle.bigvgan_ref import activation1d
    y = torch.zeros_like(x)
    for b in range(x.shape[0]):
        n = x.shape[1] if lens is None else lens[b]
        if n:
            y[b, :n] = activation1d(x[b:b + 1, :n].transpose(1, 2), al, be, np.asarray(up, np.float32), np.asarray(dn, np.float32)).transpose(1, 2)[0]
    return y


@pytest.mark.parametrize("family", sorted(R.FIRST_ACT))
def test_act_stand_in_passes_and_every_control_fails(fir, family):
    up, dn = fir
    B, T, C = R.FIRST_ACT[family]
    x, al, be = R.act_case(F32, B, T, C, R.act_seed(T, C))
    ref, e, _ = R.act_ref(x, al, be, up, dn, False)
    bound = R.act_bound(ref, e, F32)
    y = stand_in_act(x, al, be, up, dn)
    what = f"fp32 stand-in, {family} B={B} T={T} C={C}"
    print(f"fp64 | stand-in | {what} | {check(what, y, ref, bound):.3f}")
    for text, r_bad in R.act_controls(x, al, be, up, dn, R.TAP32[family]).items():
        print(f"fp64 | control | {what}: {text} | {must_fail(what, text, y, r_bad, bound):.3f}")


def test_act_stand_in_passes_lengths_ragged_and_large_arguments(fir):
    up, dn = fir
    for C in R.ACT_C:
        for T in R.act_lengths(C):
            x, al, be = R.act_case(F32, 2, T, C, R.act_seed(T, C))
            ref, e, _ = R.act_ref(x, al, be, up, dn, False)
            check(f"stand-in act C={C} T={T}", stand_in_act(x, al, be, up, dn), ref, R.act_bound(ref, e, F32))
    TT = R.AA_TT[48]
    lens = [0, 1, TT - 1, TT, TT + 1, 2 * TT + 1]
    x, al, be = R.act_case(F32, len(lens), 2 * TT + 1, 48, 7400)
    ref, e, ok = R.act_ref(x, al, be, up, dn, False, lens)
    check("stand-in ragged act", stand_in_act(x, al, be, up, dn, lens), ref, R.act_bound(ref, e, F32), ok)
    x, al, be = R.act_case(F32, 2, 300, 48, 7700, xscale=300.0, al=torch.full((48,), 0.5))
    ref, e, _ = R.act_ref(x, al, be, up, dn, False)
    r = check("stand-in act, |theta| ~ 2000 rad", stand_in_act(x, al, be, up, dn), ref, R.act_bound(ref, e, F32))
    print(f"fp64 | stand-in | act |x| <= 300, alpha 0.5 | {r:.3f}")


TANH_CASES = [(n, dt, at) for n in R.TANH_N for dt in (F32, F16, BF16) for at in (1, 0)]


def stand_in_tanh(x, apply_tanh):
    v = torch.tanh(x.float()) if apply_tanh else x.float()
    s = torch.clamp(torch.tensor(32767.0, dtype=F32) * v, -32767.0, 32767.0)
    return v, torch.trunc(s).to(torch.int16)


@pytest.mark.parametrize("n,dtype,apply_tanh", TANH_CASES)
def test_tanh_pcm_stand_in_controls_and_share(n, dtype, apply_tanh):
    x = R.tanh_inputs(n, dtype, R.tanh_seed(n, dtype), apply_tanh)
    v64, wb = R.tanh_ref(x, apply_tanh)
    wav, pcm = stand_in_tanh(x, apply_tanh)
    assert ((wav.double() - v64).abs() <= wb).all()
    lo, hi = R.pcm_allowed(x, apply_tanh)
    wrong, share = R.pcm_verdict(pcm, lo, hi)
    # the float64 reference alone stays under the cap: the seed and the input mix are chosen for it
    assert wrong == 0 and share <= R.PCM_SHARE, (wrong, share)
    assert not apply_tanh or n < 2 or share > 0          # (the saturated last element is a choice between 32766 and 32767)
    if n >= 255:
        for kw in (dict(gain=32768.0), dict(rounding="nearest")):
            wrong, _ = R.pcm_verdict(pcm, *R.pcm_allowed(x, apply_tanh, **kw))
            assert wrong > 0, kw
    if n > 1 and not apply_tanh:
        assert x.float().abs().max() > 1 and (x.float() == 1.0).any() and int(pcm.max()) == 32767 and int(pcm.min()) == -32767
    if n > 1 and apply_tanh:
        assert x.float().abs().max() == 20.0


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_tanh_loud_mix_samples_the_middle_range_and_the_stand_in_passes(dtype):
    x = R.tanh_loud_inputs(R.TANH_LOUD_N, dtype, R.TANH_SEED)
    mid = ((x.float().abs() >= 0.3) & (x.float().abs() <= 9.0)).float().mean().item()
    assert mid > 0.8 and x.float().abs().max() <= 20.0 and R.TANH_LOUD_N > 65536
    v64, wb = R.tanh_ref(x, True, R.TANH32_LOUD)
    assert ((torch.tanh(x.float()).double() - v64).abs() <= wb).all()
    assert R.TANH32_LOUD == 2 * R.TANH32_LOUD_MEASURED and R.TANH32 == 2 * R.TANH32_MEASURED and R.TANH32_LOUD < 5 * 2.0 ** -24


def test_bf16_inputs_stay_off_the_integer_lattice():
    """Without the floor the float64 reference alone breaks the cap at n past the grid cap (the derivation in tanh_inputs); with it the
    main body starts at 2^-8 and the share is that of the other types."""
    n = R.TANH_N[-1]
    x = R.tanh_inputs(n, BF16, R.TANH_SEED, True)
    body = torch.arange(n) % 4096 != 7
    assert x[body][:-1].float().abs().min() >= R.BF16_FLOOR
    raw = (R.rnd(n, seed=R.TANH_SEED) * 0.05).to(BF16)
    lo, hi = R.pcm_allowed(raw, True)
    assert (lo != hi).double().mean() > R.PCM_SHARE


# ----------------------------------------------------------------------------------------------------------- part 3
def smallest_power(leaves):
    """The smallest 2^-p (p <= 30) for which leaves(2^-p) holds, given that it holds from some power on upwards."""
    p = 1
    while p < 30 and leaves(2.0 ** -(p + 1)):
        p += 1
    assert leaves(2.0 ** -p)
    return 2.0 ** -p


def test_tap32_is_the_smallest_power(fir):
    """TAP32[family]: computed in float64 alone (the perturbed reference against the reference, under the fp32 bound) on the first case
    of each family, and held against the constants the GPU file uses."""
    got = {}
    for family, (C, N, k, d) in R.FIRST_CONV.items():
        T = R.row_tile(R.f32_conv_form(C, N, k)) + 1
        x, w, bias, off0, rk = R.conv_case(F32, 3, T, C, N, k, d, "bias", R.conv_seed(C, N, k, d, T))
        ref, mag = R.conv_ref(x, w, k, off0, d, T, bias=bias, **rk)
        bound = R.conv_bound(ref, mag, F32)
        got[family] = smallest_power(lambda e: excess(R.conv_ref(x, R.perturbed_tap(w, k // 2, e), k, off0, d, T, bias=bias, **rk)[0], ref, bound)[0] > 1)
    C, N, k, d = R.RAGGED_F32[0]
    lens = R.ragged_lens(R.row_tile(R.f32_conv_form(C, N, k)))
    vr = torch.tensor(lens, dtype=torch.int32)
    T = R.RAGGED_T
    x, w, bias, off0, rk = R.conv_case(F32, len(lens), T, C, N, k, d, "bias", R.conv_seed(C, N, k, d, T))
    ref, mag = R.conv_ref(x, w, k, off0, d, T, bias=bias, vr=vr)
    bound, valid = R.conv_bound(ref, mag, F32), (torch.arange(T)[None, :] < vr.long()[:, None])[..., None]
    got["ragged"] = smallest_power(lambda e: excess(R.conv_ref(x, R.perturbed_tap(w, k // 2, e), k, off0, d, T, bias=bias, vr=vr)[0], ref, bound, valid)[0] > 1)
    Tn, cin, c, k, u = R.UPS[0]
    x, w, bias, b2 = R.ups_case(F32, 3, Tn, cin, c, k, u, 5000 + cin, bias2=False)
    taps, off0, shift, rows, ref_of = ups_refs(x, w, bias, b2, u, 3, Tn, c)
    ref, mag = ref_of(taps)
    bound = R.conv_bound(ref, mag, F32)
    got["upsampler"] = smallest_power(lambda e: excess(ref_of(R.perturbed_tap(taps, taps.shape[0] - 1, e))[0], ref, bound)[0] > 1)
    p = R.CONV_PRE
    x, w, bias, off0, _ = R.conv_case(F32, p["B"], p["T"], p["C"], p["N"], p["k"], p["d"], "bias", 6000)
    b2 = (R.rnd(p["B"], p["N"], seed=6003) * 0.1).float()
    ref, mag = R.conv_ref(x, w, 7, off0, 1, p["T"], bias=bias, bias2=b2)
    bound = R.conv_bound(ref, mag, F32)
    got["conv_pre"] = smallest_power(lambda e: excess(R.conv_ref(x, R.perturbed_tap(w, 3, e), 7, off0, 1, p["T"], bias=bias, bias2=b2)[0], ref, bound)[0] > 1)
    up, dn = fir
    for family, (B, T, C) in R.FIRST_ACT.items():
        x, al, be = R.act_case(F32, B, T, C, R.act_seed(T, C))
        ref, e, _ = R.act_ref(x, al, be, up, dn, False)
        bound = R.act_bound(ref, e, F32)
        got[family] = smallest_power(lambda eps: excess(R.act_ref(x, al, be, up, R.perturbed_filter(dn, eps), False)[0], ref, bound)[0] > 1)
    print("TAP32:", {f: f"2^{int(math.log2(v))}" for f, v in got.items()})
    assert got == R.TAP32, {f: (math.log2(v), math.log2(R.TAP32[f])) for f, v in got.items()}
    assert all(v < 2.0 ** -12 for v in got.values())      # every one far finer than the 16-bit file's 2^-9


# ----------------------------------------------------------------------------------------------------------- part 4
def test_case_lists_reach_every_fp32_form_and_edge():
    forms = {}
    for C, N, kds in R.F32_CONV_CASES:
        for k, d in kds:
            assert (k - 1) * d <= R.CV_MAX_HALO and C % 8 == 0
            forms.setdefault(R.f32_conv_form(C, N, k), []).append((C, N, k, d))
    assert set(forms) == R.REACHABLE_F32_CONV and len(R.REACHABLE_F32_CONV) == 17
    for f, cs in forms.items():
        fixed = [k for k in (7, 11) if f.startswith(f"conv_narrow_taps<f32,") and f",{k}," in f[20:]]     # 6 d or 10 d is never 64
        assert any((k - 1) * d == (R.CV_MAX_HALO if not fixed else (fixed[0] - 1) * 5) for _, _, k, d in cs), f    # the largest halo
        assert R.row_tile(f) in (128, 256)
    assert {C for C, _, _ in R.F32_CONV_CASES} >= {8, 24, 40} and {N for _, N, _ in R.F32_CONV_CASES} >= {1, 20}
    # the forms the issue names for the vocoder's own layers
    assert R.f32_conv_form(24, 24, 7) == "conv_narrow<f32,2,2>" and R.f32_conv_form(48, 48, 11) == "conv_narrow<f32,3,3>"
    assert R.f32_conv_form(96, 96, 3) == "gemm_conv<f32,2,2,4,3,2,64,persist>" and R.f32_conv_form(24, 1, 7) == "conv_narrow<f32,2,1>"
    assert R.f32_conv_form(16, 32, 3) == "conv_narrow_taps<f32,1,2,3,4,4>" and R.f32_conv_form(32, 48, 11) == "conv_narrow_taps<f32,2,3,11,2,4>"
    assert R.row_tile("conv_narrow_taps<f32,2,3,11,2,4>") == 128 and R.row_tile("conv_narrow_taps<f32,1,2,3,4,4>") == 256
    assert R.row_tile("gemm_conv<f32,4,1,4,3,2,64>") == 256 and R.row_tile("gemm_conv<f32,2,2,4,2,2,64,persist>") == 128
    for fam, (C, N, k, d) in R.FIRST_CONV.items():
        assert C % R.KS32 == 8, fam          # the K-padding control needs a padded last k-step
    assert {R.aa_cs(C) for C in R.ACT_C} == set(R.AA_TT) and R.TANH_N[-1] > R.TANH_GRID_CAP
