"""fp64 parity of every fp32 vocoder kernel form, element by element: the forms the parity mode runs and the 16-bit modes are judged by.

dispatch_conv<float> with taps > 1 (conv_narrow, conv_narrow_taps and the five tiled forms of Elem<float>: E = 4, KS = 16,
v_mfma_f32_16x16x4_f32), aa_snake_btc_kernel<float, CS>, aa_snake_bct_kernel<float> and tanh_pcm_kernel<T>.  References, bounds,
controls, the dispatch rule (REACHABLE_F32_CONV) and the case lists are tests/vocoder_refs.py; tests/test_vocoder_refs_cpu.py holds
them to torch's float64 operators and to an fp32 stand-in without a GPU.  Built like tests/test_vocoder_kernels_gpu.py: one launch
per case on operands already in fp32, the sentinel 7.0 where nothing may be written, `itts_last_kernel()` asserted and collected in
PINNED (convolutions with taps > 1: held equal to REACHABLE_F32_CONV at the end of the file) or PINNED_OTHER (the 1-tap up-samplers'
plain-GEMM forms and the activation forms), one `fp64 | kind | case | ratio` line per check with -s
(profiles/vocoder_fp32_fp64.txt).  The first case of every family runs the negative controls, which only re-evaluate the reference.
No fp32 call may name conv_narrow_lds (compiled for 2-byte types only) or an MFMA activation form.

Activation: act_bound(ref, E, F32) with E from act_ref(..., mfma=False) and the hardware-sine allowance EHW = 2^-19 kept as the upper
bound of libm sinf (vocoder_refs.py says why).

`test_forward_*` record the signatures and forms of one eager fp32 BigVGAN.forward on the synthetic full-size checkpoint (batch 2,
9 latent frames).  For taps > 1 the fp32 dispatch depends on (Cin, N, taps) alone -- dispatch_narrow<float> reads p.Cin, p.N, p.taps,
p.KT, p.NT and nothing else once `if constexpr (sizeof(T) == 2)` has removed the conv_narrow_lds branch, and the tiled tail of
dispatch_conv (`if (p.N % 128 == 0) return launch_conv<T, 1, 4, 8, 2, 2, CV_MAX_HALO>...`) reads p.N --, so T, the batch, the dilation
and the epilogue of a signature can shrink without leaving its form: every distinct signature runs against fp64 at its own small T."""
import math

import pytest
import torch

import vocoder_refs as R
import weights
from fp64_check import bad, note, ok, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PINNED = set()            # convolution forms (taps > 1) pinned to fp64
PINNED_OTHER = set()      # plain-GEMM forms of the 1-tap up-samplers and activation forms pinned to fp64


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fir():
    from indextts.BigVGAN.models import kaiser_sinc_filter
    f = kaiser_sinc_filter()
    return f, f


def form(nat, expect=None, pin=PINNED):
    f = nat.last_kernel()
    assert "conv_narrow_lds" not in f and "mfma" not in f, f"an fp32 call dispatched {f!r}"
    if expect is not None:
        assert f == expect or (expect.endswith("*") and f.startswith(expect[:-1])), f"dispatched {f!r}, expected {expect!r}"
    if pin is not None:
        pin.add(f)
    return f


# ------------------------------------------------------------------------------------------------- convolution
def run_conv(nat, B, T, C, N, k, d, epi, family=None, vr=None, expect=None, pin=PINNED, seed=None):
    """One 'same' fp32 convolution with the epilogue `epi` against fp64; family: run the controls with TAP32[family]."""
    x, w, bias, off0, rk = R.conv_case(F32, B, T, C, N, k, d, epi, R.conv_seed(C, N, k, d, T) if seed is None else seed, device=DEV)
    y = rk["yprev"].clone() if "yprev" in rk else torch.full((B, T, N), 7.0, dtype=F32, device=DEV)
    kw = {n: rk[n] for n in ("resid", "scale", "bias2") if n in rk}
    nat.gemm_conv(F32, B, T, T, C, N, nat.pack_weight(w), x, y, taps=k, off0=off0, dil=d, bias=bias, valid_rows=vr,
                  accumulate="yprev" in rk, **kw)
    f = form(nat, R.f32_conv_form(C, N, k) if expect is None else expect, pin)
    what = f"{f} B={B} T={T} C={C} N={N} k={k} d={d} {epi}" + ("" if vr is None else f" lens={vr.tolist()}")
    ref, mag = R.conv_ref(x, w, k, off0, d, T, bias=bias, vr=vr, **rk)
    bound = R.conv_bound(ref, mag, F32)
    valid = None if vr is None else (torch.arange(T, device=DEV)[None, :] < vr.long()[:, None])[..., None]
    ok(what, y, ref, bound, valid)
    if vr is not None and "yprev" not in rk:     # y started as the sentinel: whole tiles past a length are skipped and it stays
        for b, n in enumerate(vr.tolist()):
            if n + 512 + (k - 1) * d < T:
                assert (y[b, n + 512 + (k - 1) * d:] == 7.0).all(), (what, b)
    if family is not None:
        for text, r_bad in R.conv_controls(x, w, k, off0, d, T, bias, rk, R.TAP32[family] if epi == "bias" else None, vr).items():
            bad(what, text, y, r_bad, bound, valid)
    return f


FIRST = {v[:3]: fam for fam, v in R.FIRST_CONV.items()}


@pytest.mark.parametrize("C,N,kds", R.F32_CONV_CASES, ids=lambda v: str(v) if isinstance(v, int) else "kd%d" % len(v))
def test_conv_forms_fp64(nat, C, N, kds):
    """T = 1 and one below, on and one above the form's row tile, every epilogue of EPI_MATRIX, each (k, d) of the case."""
    for k, d in kds:
        tile = R.row_tile(R.f32_conv_form(C, N, k))
        fam = FIRST.get((C, N, k)) if (C, N, k, d) in R.FIRST_CONV.values() else None
        for T in (1, tile - 1, tile, tile + 1):
            for epi in R.EPI_MATRIX:
                run_conv(nat, 3, T, C, N, k, d, epi, family=fam if (T == tile + 1 and epi in R.CONTROL_EPIS) else None)


@pytest.mark.parametrize("i", range(len(R.RAGGED_F32)))
def test_ragged_conv_fp64_each_element_at_its_own_length(nat, i):
    C, N, k, d = R.RAGGED_F32[i]
    lens = R.ragged_lens(R.row_tile(R.f32_conv_form(C, N, k)))
    vr = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for epi in ("bias", "resid", "resid_acc_third"):
        run_conv(nat, len(lens), R.RAGGED_T, C, N, k, d, epi, family="ragged" if (i == 0 and epi in R.CONTROL_EPIS) else None, vr=vr)


def run_upsampler(nat, B, Tn, cin, c, k, u, seed, bias2, controls=False, expect=None, record=True):
    x, w, bias, b2 = R.ups_case(F32, B, Tn, cin, c, k, u, seed, bias2, device=DEV)
    taps, off0, shift = R.convtr_taps(w, u)
    nt = taps.shape[0]
    Tu, rows = Tn * u, Tn + nt - 1
    y = torch.full((B, Tu, c), 7.0, dtype=F32, device=DEV)
    nat.gemm_conv(F32, B, Tn, rows, cin, u * c, nat.pack_weight(taps), x, y, taps=nt, off0=off0, dil=1, bias=bias, bias2=b2,
                  y_bstride=Tu * c, y_shift=shift, y_limit=Tu * c)
    want = R.f32_conv_form(cin, u * c, nt) if nt > 1 else "gemm_plain<f32,*"
    f = form(nat, want if expect is None else expect, (PINNED if nt > 1 else PINNED_OTHER) if record else None)

    def ref_of(xx, tp):
        acc, mag = R.conv_ref(xx, tp, nt, off0, 1, rows, bias=bias, bias2=b2)
        return R.ups_slice(acc, shift, B, Tu, c), R.ups_slice(mag, shift, B, Tu, c)

    ref, mag = ref_of(x, taps)
    bound = R.conv_bound(ref, mag, F32)
    what = f"{f} upsampler B={B} Tn={Tn} {cin}->{c} k={k} u={u} (Cin taps = {cin * nt})"
    ok(what, y, ref, bound)
    if controls:
        eps = R.TAP32["upsampler"]
        bad(what, f"one weight tap off by 2^{int(math.log2(eps))} relative", y, ref_of(x, R.perturbed_tap(taps, nt - 1, eps))[0], bound)
        bad(what, "x rounded to fp16 before the product", y, ref_of(R.x_through_fp16(x), taps)[0], bound)
    return f


@pytest.mark.parametrize("i", range(len(R.UPS)))
def test_upsampler_fp64(nat, i):
    Tn, cin, c, k, u = R.UPS[i]
    run_upsampler(nat, 3, Tn, cin, c, k, u, 5000 + cin, bias2=(cin >= 768), controls=(i == 0))


def run_conv_pre(nat, B, T, seed=6000, controls=False, expect="gemm_conv<f32,1,4,8,2,2,64>", pin=PINNED):
    p = R.CONV_PRE
    x, w, bias, off0, _ = R.conv_case(F32, B, T, p["C"], p["N"], p["k"], p["d"], "bias", seed, device=DEV)
    b2 = (rnd(B, p["N"], seed=seed + 3, device=DEV) * 0.1).float()
    y = torch.full((B, T, p["N"]), 7.0, dtype=F32, device=DEV)
    nat.gemm_conv(F32, B, T, T, p["C"], p["N"], nat.pack_weight(w), x, y, taps=7, off0=off0, dil=1, bias=bias, bias2=b2)
    f = form(nat, expect, pin)
    ref, mag = R.conv_ref(x, w, 7, off0, 1, T, bias=bias, bias2=b2)
    bound = R.conv_bound(ref, mag, F32)
    what = f"{f} conv_pre B={B} T={T} 1280->1536 k=7 (Cin taps = 8960)"
    ok(what, y, ref, bound)
    if controls:
        eps = R.TAP32["conv_pre"]
        bad(what, f"one weight tap off by 2^{int(math.log2(eps))} relative", y, R.conv_ref(x, R.perturbed_tap(w, 3, eps), 7, off0, 1, T, bias=bias, bias2=b2)[0], bound)
        bad(what, "x rounded to fp16 before the product", y, R.conv_ref(R.x_through_fp16(x), w, 7, off0, 1, T, bias=bias, bias2=b2)[0], bound)


def test_conv_pre_fp64(nat):
    run_conv_pre(nat, R.CONV_PRE["B"], R.CONV_PRE["T"], controls=True)


# ------------------------------------------------------------------------------------------------- activation
def run_act(nat, fir, B, T, C, seed, expect, family=None, lens=None, xscale=1.0, al=None, layout=0, pin=PINNED_OTHER):
    up, dn = fir
    x, al, be = R.act_case(F32, B, T, C, seed, xscale=xscale, al=al, device=DEV)
    vr = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    if layout == 0:
        y = torch.full_like(x, 7.0)
        nat.aa_snake(x, al, be, up, dn, layout=0, out=y, valid_rows=vr)
    else:
        y = nat.aa_snake(x.transpose(1, 2).contiguous(), al, be, up, dn, layout=1).transpose(1, 2)
    f = form(nat, expect, pin)
    what = f"{f} B={B} T={T} C={C}" + ("" if lens is None else f" lens={lens}") + (f" |x|<={xscale}" if xscale != 1.0 else "")
    ref, e, okm = R.act_ref(x, al, be, up, dn, False, lens)
    bound = R.act_bound(ref, e, F32)
    ok(what, y, ref, bound, okm)
    if lens is not None:
        assert (y[~okm.expand_as(y)] == 7.0).all(), f"{what}: rows past a length were written"
    if family is not None:
        for text, r_bad in R.act_controls(x, al, be, up, dn, R.TAP32[family], lens).items():
            bad(what, text, y, r_bad, bound, okm)


@pytest.mark.parametrize("C", R.ACT_C)
def test_act_btc_fp64(nat, fir, C):
    cs = R.aa_cs(C)
    TT = R.AA_TT[cs]
    first = R.FIRST_ACT["act_btc"]
    for T in R.act_lengths(C):
        run_act(nat, fir, 2, T, C, R.act_seed(T, C), f"aa_snake_btc<f32,{cs}>", family="act_btc" if (2, T, C) == first else None)
    lens = [0, 1, TT - 1, TT, TT + 1, 2 * TT + 1]
    run_act(nat, fir, len(lens), 2 * TT + 1, C, 7400 + C, f"aa_snake_btc<f32,{cs}>", lens=lens)


@pytest.mark.parametrize("T", R.BCT_T)
def test_act_bct_fp64(nat, fir, T):
    B, _, C = R.FIRST_ACT["act_bct"]
    run_act(nat, fir, B, T, C, R.act_seed(T, C), "aa_snake_bct<f32>", family="act_bct" if T == R.FIRST_ACT["act_bct"][1] else None, layout=1)


def test_act_large_arguments(nat, fir):
    """|u e^alpha| up to ~2 000 rad: libm sinf's own range reduction is what is under test."""
    run_act(nat, fir, 2, 300, 48, 7700, "aa_snake_btc<f32,48>", xscale=300.0, al=torch.full((48,), 0.5, device=DEV))
    run_act(nat, fir, 2, 300, 384, 7701, "aa_snake_btc<f32,64>", xscale=300.0, al=torch.full((384,), 0.5, device=DEV))


def test_act_fp32_never_takes_the_mfma_form(nat, fir):
    """B T >= 32768 at C = 48 is where fp16 switches to aa_snake_mfma<3>; fp32 stays on the VALU form."""
    run_act(nat, fir, 1, 32768, 48, 7800, "aa_snake_btc<f32,48>")


# ------------------------------------------------------------------------------------------------- tanh_pcm
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("n", R.TANH_N)
def test_tanh_pcm_fp64(nat, dtype, n):
    for apply_tanh in (1, 0):
        x = R.tanh_inputs(n, dtype, R.tanh_seed(n, dtype), apply_tanh, device=DEV)
        v64, wb = R.tanh_ref(x, apply_tanh)
        lo, hi = R.pcm_allowed(x, apply_tanh)
        what = f"tanh_pcm<{'f32' if dtype == F32 else 'f16' if dtype == F16 else 'bf16'}> n={n} apply_tanh={apply_tanh}"
        for outs in ("wav", "pcm", "both"):
            wav = torch.full((n,), 7.0, dtype=F32, device=DEV) if outs != "pcm" else None
            pcm = torch.full((n,), 7, dtype=torch.int16, device=DEV) if outs != "wav" else None
            nat.tanh_pcm(x, wav=wav, pcm=pcm, apply_tanh=bool(apply_tanh))
            if wav is not None:
                err = (wav.double() - v64).abs()
                if apply_tanh:
                    note("measure", f"{what} {outs}: worst |tanhf - tanh64| in units of 2^-24 (TANH32 = 2 x {R.TANH32_MEASURED * 2 ** 24:.3f})", err.max().item() * 2.0 ** 24)
                    ok(f"{what} {outs} wav", wav, v64, wb)
                else:
                    assert torch.equal(wav, x.float()), what
            if pcm is not None:
                wrong, share = R.pcm_verdict(pcm, lo, hi)
                note("case", f"{what} {outs} pcm: share of elements with a choice (cap {R.PCM_SHARE})", share)
                assert wrong == 0 and share <= R.PCM_SHARE, (what, wrong, share)
                if n >= 255 and outs == "both":
                    for text, kw in (("32768 in place of 32767", dict(gain=32768.0)), ("round to nearest in place of truncation", dict(rounding="nearest"))):
                        wrong, _ = R.pcm_verdict(pcm, *R.pcm_allowed(x, apply_tanh, **kw))
                        note("control", f"{what}: {text}: elements outside", wrong)
                        assert wrong > 0, (what, text)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_tanh_loud_wav_fp64(nat, dtype):
    """tanhf where its error is largest: N(0, 1.5), wav only, against tanh64 under ulp_f32 + TANH32_LOUD (its own measured figure)."""
    n = R.TANH_LOUD_N
    x = R.tanh_loud_inputs(n, dtype, R.TANH_SEED, device=DEV)
    v64, wb = R.tanh_ref(x, True, R.TANH32_LOUD)
    wav = torch.full((n,), 7.0, dtype=F32, device=DEV)
    nat.tanh_pcm(x, wav=wav, pcm=None, apply_tanh=True)
    what = f"tanh_pcm<{'f32' if dtype == F32 else 'f16' if dtype == F16 else 'bf16'}> n={n} loud mix N(0, 1.5)"
    note("measure", f"{what}: worst |tanhf - tanh64| in units of 2^-24 (TANH32_LOUD = 2 x {R.TANH32_LOUD_MEASURED * 2 ** 24:.3f})",
         (wav.double() - v64).abs().max().item() * 2.0 ** 24)
    ok(f"{what} wav", wav, v64, wb)


# ------------------------------------------------------------------------------------------------- the real forward
@pytest.fixture(scope="module")
def forward_record(nat):
    """Signatures and forms of one eager fp32 BigVGAN.forward (synthetic full-size checkpoint, batch 2, 9 latent frames)."""
    from indextts.BigVGAN.models import BigVGAN
    from indextts.utils.config import Config
    v = BigVGAN(Config(weights.reference_config()["bigvgan"]))
    v.load_state_dict(weights.bigvgan_state_dict())
    v.to(DEV).to(F32).remove_weight_norm()
    B, Tn = 2, 9
    lat = rnd(B, Tn, 1280, seed=9000, device=DEV).float()
    spk = rnd(B, 1, 512, seed=9001, device=DEV).float() * 0.1
    rec = []
    g0, a0 = nat.gemm_conv, nat.aa_snake

    def g(dtype, B, Tin, Tout, Cin, N, wp, x, y, **kw):
        g0(dtype, B, Tin, Tout, Cin, N, wp, x, y, **kw)
        rec.append(("conv", dtype, B, Tin, Tout, Cin, N, kw.get("taps", 1), kw.get("off0", 0), kw.get("dil", 1),
                    kw.get("bias2") is not None, kw.get("resid") is not None, bool(kw.get("accumulate", False)),
                    float(kw.get("scale", 1.0)), int(kw.get("y_shift", 0)), y.shape[-1], nat.last_kernel()))

    def a(x, al, be, up, dn, layout=0, out=None, valid_rows=None):
        y = a0(x, al, be, up, dn, layout=layout, out=out, valid_rows=valid_rows)
        rec.append(("act", x.dtype, x.shape[0], x.shape[1], x.shape[2], nat.last_kernel()))
        return y

    nat.gemm_conv, nat.aa_snake = g, a
    try:
        with torch.no_grad():
            v(lat, speaker_embedding=spk)
        torch.cuda.synchronize()
    finally:
        nat.gemm_conv, nat.aa_snake = g0, a0
    del v
    return rec


def test_forward_signatures_fp64(nat, fir, forward_record):
    """Every distinct (C_in, N, taps, dilation, epilogue, form) of the fp32 forward at its own small T, against fp64."""
    seen = set()
    for i, r in enumerate(forward_record):
        assert r[1] == F32, r
        if r[0] == "act":
            _, _, B, T, C, f = r
            if ("act", C, f) not in seen:
                seen.add(("act", C, f))
                assert f == f"aa_snake_btc<f32,{R.aa_cs(C)}>", r
                run_act(nat, fir, B, min(T, 2 * R.AA_TT[R.aa_cs(C)] + 3), C, 9100 + i, f, pin=None)
            continue
        _, _, B, Tin, Tout, Cin, N, taps, off0, dil, has_b2, has_r, acc, scale, y_shift, c, f = r
        key = (Cin, N, taps, dil, off0, has_b2, has_r, acc, scale, y_shift, f)
        if key in seen:
            continue
        seen.add(key)
        if taps > 1:
            assert f == R.f32_conv_form(Cin, N, taps), r
        if c != N:                               # an upsampler: [Tin (+1) rows][u*c] stored shifted into [u*Tin][c]
            u = N // c
            k = 2 * u if taps == 2 else u
            assert Tout == Tin + (taps - 1) and y_shift == -((k - u) // 2) * c, r
            run_upsampler(nat, B, min(Tin, 40), Cin, c, k, u, 9200 + i, bias2=has_b2, expect=f if taps > 1 else None, record=False)
            continue
        if has_b2:                               # conv_pre: the conditioning bias, no residual
            assert (Cin, N, taps) == (1280, 1536, 7) and not has_r, r
            run_conv_pre(nat, B, Tin, seed=9300 + i, expect=f, pin=None)
            continue
        epi = [e for e, v in R.EPIS.items() if v == (has_r, acc, scale if scale == 1.0 else 1.0 / 3.0, False)]
        assert len(epi) == 1 and abs(scale - R.EPIS[epi[0]][2]) < 1e-7 and off0 == -((taps - 1) * dil // 2), r
        run_conv(nat, B, min(Tin, R.row_tile(f) + 9), Cin, N, taps, dil, epi[0], expect=f, pin=None, seed=9400 + i)
    assert len(seen) >= 20


def test_forward_forms_are_pinned(nat, forward_record):
    """Every kernel form the fp32 forward launched is pinned by the edge matrix above (which runs first, in file order)."""
    used = sorted({r[-1] for r in forward_record})
    print("kernel forms of the fp32 forward:", ", ".join(used))
    assert not any("conv_narrow_lds" in f or "mfma" in f for f in used), used
    missing = [f for f in used if f not in PINNED | PINNED_OTHER]
    assert not missing, f"forms of the fp32 forward no edge case pins: {missing} (used: {used})"


def test_every_reachable_fp32_conv_form_is_pinned():
    """PINNED == REACHABLE_F32_CONV: every float instantiation dispatch_conv<float> can return for taps > 1, and no other."""
    assert PINNED == R.REACHABLE_F32_CONV, (sorted(R.REACHABLE_F32_CONV - PINNED), sorted(PINNED - R.REACHABLE_F32_CONV))
