"""float64 references of the vocoder kernels -- itts_gemm_conv with taps > 1 (and the up-samplers' 1- and 2-tap rewrites), the
anti-aliased SnakeBeta activation itts_aa_snake_fwd and itts_tanh_pcm --, their per-element bounds, their negative-control builders and,
for the fp32 forms, the dispatch rule, the case lists and the operand generators.  Device-agnostic plain torch: every function works on
the device of its operands and makes no call into the library, so tests/test_vocoder_refs_cpu.py can hold each reference to torch's own
float64 operators, let a plain float32 evaluation stand in for the kernel and show that every control leaves its bound, without a GPU.
tests/test_vocoder_kernels_gpu.py (16-bit forms) and tests/test_vocoder_fp32_kernels_gpu.py (fp32 forms) both import from here.

Convolution (every form accumulates exact products in fp32 -- 16-bit operands: v_mfma_f32_16x16x32; fp32 operands: Elem<float>, four
v_mfma_f32_16x16x4_f32 per k-step of KS = 16 channels -- and rounds once to the storage type):
      |y - ref| <= ulp_T(ref) + CHAIN * S,   S = |scale| * (sum_{j,c} |x w| + |bias| + |bias2| + |resid|) + |y_prev|
  CHAIN = 2^-21 is the project's fp32-chain figure, imported from tests/plain_gemm_refs.py, which applies it to its fp32 cases; at
  T = fp32 nothing else changes: resid and y_prev are fp32 values, there is no 16-bit rounding of them to model, and ulp_f32(ref) covers
  the single final rounding (half an ulp) with half an ulp to spare.  CHAIN is not re-derived or raised for the vocoder's deep
  reductions (Cin * taps = 1536 * 8 and 1280 * 7): profiles/vocoder_fp32_fp64.txt has their measured ratios.

Activation: see `act_bound`.  The fp32 form (aa_snake_btc_kernel<float, CS>, aa_snake_bct_kernel<float>) is held to act_bound(ref, E, F32)
  with E from act_ref(..., mfma=False): fp32 never takes the MFMA form.  Its sine is libm sinf (aa_sin<float>), for which the hardware-sine
  allowance EHW = 2^-19 absolute is kept unchanged as an upper bound: sinf's own error is a few ulp of a value <= 1 (< 2^-22), there is
  no documented tighter figure for this library build to cite, and EHW enters E only through ib * 2 EHW next to 2^-20 |theta|.

tanh_pcm (tanh_pcm_kernel<T>: v = tanhf(float(x)), wav = v, pcm = (int16) clamp(32767 v, +-32767), truncation toward zero):
      apply_tanh = 1:   |wav - tanh64(x)| <= ulp_f32(ref) + TANH32
      apply_tanh = 0:   wav == float(x) exactly (the bound is 0), pcm == trunc(clamp(fl32(32767 x))) exactly: 32767 x is exact in float64
                        (15 x 24 bits) and fl32 of it is the kernel's one rounding
  TANH32 is tanhf's error.  The citable ceiling is the OpenCL C specification's 5 ulp for tanh (OCML implements that profile), 5 * 2^-24
  absolute for |v| < 1; measured on an MI355X against float64 over the inputs of `tanh_inputs` (every size of TANH_N, fp32 / fp16 /
  bf16 inputs) the worst |tanhf(x) - tanh64(x)| is TANH32_MEASURED = 0.653 * 2^-24 = 3.89e-8, and TANH32 allows twice that, 7.78e-8
  (profiles/vocoder_fp32_fp64.txt has both numbers; the GPU test prints the measurement again with every run).  That mix is quiet, as
  the PCM cap requires (`tanh_inputs`), and samples tanh's middle range thinly; `tanh_loud_inputs` (N(0, 1.5), wav only) samples it
  densely and is held to its own figure, TANH32_LOUD = 2 * TANH32_LOUD_MEASURED, measured the same way.
  pcm with apply_tanh = 1: equal to trunc(clamp(32767 v64)) except where 32767 v64 lies within W = 32767 * (the wav bound) of an
  integer, where either neighbour is allowed -- `pcm_allowed` returns trunc(clamp(t - W)) and trunc(clamp(t + W)), which differ exactly
  there (and at the clamp, where a saturated tanhf may give 32766 or 32767).  That share is capped at PCM_SHARE = 1 % of the elements.

Negative controls: builders that return operands wrong in one small way (rows shifted by one at a tile boundary, one tap off by a
relative eps, two channels exchanged, zero instead of replicate padding, alpha and beta swapped; fp32 only: x rounded to fp16 before the
product, the K-padding columns of the last k-step read from past the row's end).  A control re-evaluates the reference on them; the
kernel's output is compared with it under the same bound and must fail.  The 16-bit file perturbs a tap by 2^-9, a thousand times
coarser than an fp32 bound; the fp32 arms use TAP32[family], the smallest power of two at which the perturbed float64 reference
itself leaves the bound on at least one element of the first case of that family (FIRST_CONV, UPS[0], CONV_PRE, FIRST_ACT; computed
in float64 alone and asserted by tests/test_vocoder_refs_cpu.py)."""
import math

import numpy as np
import torch

from fp64_check import rnd, ulp
from plain_gemm_refs import CHAIN

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CV_MAX_HALO = 64        # gemm_conv.hip: (taps - 1) * dil may not exceed it
KS32 = 16               # k-step of the fp32 MFMA forms (Elem<float>::KS)


# ------------------------------------------------------------------------------------------------- convolution
def conv_ref(x, w, taps, off0, dil, Tout, bias=None, bias2=None, resid=None, yprev=None, scale=1.0, vr=None):
    """fp64 y[b,t,n] = (sum_j sum_c x[b, t+off0+j*dil, c] W[j,c,n] + bias[n] + bias2[b,n] + resid) * scale + y_prev, zero
    padding (and rows past vr[b] read as zeros); returns (ref, S) with S the sum of |terms| of the bound."""
    B, Tin, Cin = x.shape
    N = w.shape[2]
    dev = x.device
    xd = x.double()
    if vr is not None:
        xd = xd * (torch.arange(Tin, device=dev)[None, :] < vr.long()[:, None])[..., None]
    wd = w.double()
    acc = torch.zeros(B, Tout, N, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(acc)
    for j in range(taps):
        s = off0 + j * dil
        lo, hi = max(0, -s), min(Tout, Tin - s)
        if hi > lo:
            xs = xd[:, lo + s:hi + s]
            acc[:, lo:hi] += xs @ wd[j]
            mag[:, lo:hi] += xs.abs() @ wd[j].abs()
    for t in (bias, None if bias2 is None else bias2[:, None, :], resid):
        if t is not None:
            acc = acc + t.double()
            mag = mag + t.double().abs()
    sc = float(np.float32(scale))
    acc, mag = acc * sc, mag * abs(sc)
    if yprev is not None:
        acc, mag = acc + yprev.double(), mag + yprev.double().abs()
    return acc, mag


def conv_bound(ref, mag, dtype):
    return ulp(ref, dtype) + CHAIN * mag


# epilogues: (residual, accumulate into y, scale, per-batch bias2); the vocoder's second convolutions use "resid",
# "resid_third" (first AMP block of a stage) and "resid_acc_third" (the other two), never with bias2
EPIS = {"bias": (False, False, 1.0, False), "resid": (True, False, 1.0, False), "resid_third": (True, False, 1.0 / 3.0, False),
        "resid_acc_third": (True, True, 1.0 / 3.0, False), "bias2_resid_acc": (True, True, 1.0 / 3.0, True)}
EPI_MATRIX = ("bias", "resid", "resid_acc_third", "bias2_resid_acc")


def ups_slice(t, shift, B, Tu, c):
    """The up-sampler's output [B][Tu][c] out of the convolution over [rows][u * c] columns: the flat row-major image of a batch
    element, shifted by y_shift (= -shift elements dropped at its head) and cut at y_limit = Tu * c."""
    lo = -shift
    return t.reshape(B, -1)[:, lo:lo + Tu * c].reshape(B, Tu, c)


def shifted_rows(x, tb):
    """x [B][T][C] with rows tb .. T-2 replaced by their successors: the input shifted by one row from row tb on."""
    xs = x.clone()
    xs[:, tb:-1] = x[:, tb + 1:]
    return xs


def perturbed_tap(w, j, eps):
    """float64 copy of the taps w [taps][Cin][N] with tap j off by eps relative."""
    wb = w.double().clone()
    wb[j] *= 1 + eps
    return wb


def swapped_last(t):
    """t with entries 0 and 1 of its last dimension exchanged (two output channels of a weight, two channels of an input)."""
    tb = t.clone()
    tb[..., [0, 1]] = t[..., [1, 0]]
    return tb


def perturbed_filter(dn, eps):
    """float64 copy of the 12 down-filter taps with the largest one off by eps relative."""
    dnb = np.array(dn, dtype=np.float64)
    dnb[int(np.argmax(np.abs(dn)))] *= 1 + eps
    return dnb


# ------------------------------------------------------------------------------------------------- activation
# absolute error allowance of the hardware sine (v_sin_f32; the MFMA form reduces its argument to [0, 1) revolutions first); kept as
# the upper bound of libm sinf in the fp32 form (module docstring)
EHW = 2.0 ** -19


def act_ref(x, al, be, up, dn, mfma, lens=None, end_pad="replicate"):
    """fp64 anti-aliased SnakeBeta of x [B,T,C] (storage type), channels last, each element at its own length.

    u[2q] = 2 sum_{d=-3..2} x[q+d] up[5-2d], u[2q+1] = 2 sum_{d=-2..3} x[q+d] up[6-2d] (x index clamped: replicate padding);
    s = u + sin^2(u e^alpha) / (e^beta + 1e-9);  y[t] = sum_j down[j] s[clamp(2t + j - 5, 0, 2n - 1)].
    mfma: s is rounded to fp16 before the down filter, as the MFMA form does.  Returns (y_ref, E, ok_len mask) with E the
    fp32-level error budget of `act_bound`."""
    B, T, C = x.shape
    dev = x.device
    ys, es = torch.zeros(B, T, C, dtype=torch.float64, device=dev), torch.zeros(B, T, C, dtype=torch.float64, device=dev)
    up2 = [2.0 * float(np.float32(v)) for v in up]
    dn_ = [float(np.float32(v)) for v in dn]
    ea = torch.exp(al.double())
    ib = 1.0 / (torch.exp(be.double()) + float(np.float32(1e-9)))
    groups = [(list(range(B)), T)] if lens is None else [([b], n) for b, n in enumerate(lens) if n > 0]
    for bs, n in groups:
        xd = x[bs, :n].double()
        q = torch.arange(n, device=dev)
        if end_pad == "replicate":
            xat = lambda dd: xd[:, torch.clamp(q + dd, 0, n - 1)]
        else:     # negative control: zero padding past the end
            xat = lambda dd: torch.where((q + dd < n)[None, :, None], xd[:, torch.clamp(q + dd, 0, n - 1)], torch.zeros_like(xd))
        ue = sum(xat(dd) * up2[5 - 2 * dd] for dd in range(-3, 3))
        uo = sum(xat(dd) * up2[6 - 2 * dd] for dd in range(-2, 4))
        uae = sum(xat(dd).abs() * abs(up2[5 - 2 * dd]) for dd in range(-3, 3))
        uao = sum(xat(dd).abs() * abs(up2[6 - 2 * dd]) for dd in range(-2, 4))
        xae = sum(xat(dd).abs() for dd in range(-3, 3))
        xao = sum(xat(dd).abs() for dd in range(-2, 4))
        il = lambda a, b: torch.stack([a, b], 2).reshape(len(bs), 2 * n, C)
        u, ua, xa = il(ue, uo), il(uae, uao), il(xae, xao)
        th = u * ea
        s = u + ib * torch.sin(th) ** 2
        # fp32-level error of the kernel's s: up-filter sums (+ the hi/lo split of the fp16 tap matrices in the MFMA form)
        # carried through ds/du = 1 + (ib e^alpha) sin 2θ, the phase (fp32 e^alpha, the products and the 1/2pi scaling:
        # a few 2^-24 |θ|), the hardware sine (EHW), and the fp32 roundings of s itself
        du = 2.0 ** -20 * ua + ((2.0 ** -22 * ua + 2.0 ** -25 * xa) if mfma else 0.0)
        e_s = du * (1 + ib * ea) + ib * (2.0 ** -20 * th.abs() + 2 * EHW) + 2.0 ** -21 * (u.abs() + ib)
        if mfma:
            s16 = s.to(F16).double()
            near = (0.5 * ulp(s, F16) - (s - s16).abs()) <= 2 * e_s     # may round to the neighbour: one fp16 ulp more
            extra = torch.where(near, ulp(s, F16), torch.zeros_like(s))
            s = s16
        else:
            extra = torch.zeros_like(s)
        m = torch.arange(n, device=dev)
        if end_pad == "replicate":
            sat = lambda j: s[:, torch.clamp(2 * m + j - 5, 0, 2 * n - 1)]
        else:
            sat = lambda j: torch.where((2 * m + j - 5 < 2 * n)[None, :, None], s[:, torch.clamp(2 * m + j - 5, 0, 2 * n - 1)],
                                        torch.zeros_like(s[:, :n]))
        at = lambda a, j: a[:, torch.clamp(2 * m + j - 5, 0, 2 * n - 1)]
        y = sum(dn_[j] * sat(j) for j in range(12))
        sa = sum(abs(dn_[j]) * at(s, j).abs() for j in range(12))
        e = 2.0 ** -20 * sa + sum(abs(dn_[j]) * (at(e_s, j) + at(extra, j)) for j in range(12))
        if mfma:      # the down filter's hi/lo tap split
            e = e + sum((2.0 ** -22 * abs(dn_[j]) + 2.0 ** -25) * at(s, j).abs() for j in range(12))
        ys[bs, :n] = y
        es[bs, :n] = e
    ok = None
    if lens is not None:
        ok = (torch.arange(T, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None])[..., None]
    return ys, es, ok


def act_bound(ref, e, dtype):
    """Derivation.  The kernel's value before its last rounding differs from the reference (same operands, float64) by
    at most E:  the up-filter sums (fp32 fma chains, or MFMAs with fp16 hi + lo tap matrices exact to ~2^-22 relative and
    2^-25 absolute), carried into s through ds/du = 1 + (ib e^alpha) sin(2θ);  the phase error of θ = u e^alpha (fp32
    e^alpha, product, 1/2pi scaling: 2^-20 |θ| is ~4x their sum) and the hardware sine;  the fp32 roundings of s;  the
    down-filter sums (2^-20 sum |down s|: 12 fp32 roundings, or the hi/lo MFMAs).  In the MFMA form s is rounded to fp16
    in LDS: the reference rounds it too, and where the reference s lies within (2x its fp32 error) of an fp16 rounding
    midpoint the kernel may round it the other way -- one fp16 ulp of s times |down[j]| more.  The final rounding to the
    storage type adds half an ulp at the reference value.  Bound = ulp/2 + 2 E (2: slack on the fp32-level constants).
    fp32 storage: the same with ulp_f32 and the E of mfma=False; the sine is libm sinf, for which EHW is kept (module docstring)."""
    return 0.5 * ulp(ref, dtype) + 2.0 * e


# ================================================================================================= the fp32 forms
# Negative-control magnitudes of the fp32 arms (module docstring; asserted by test_vocoder_refs_cpu.py::test_tap32_is_the_smallest_power)
TAP32 = {"narrow": 2.0 ** -19, "narrow_taps": 2.0 ** -18, "tiled": 2.0 ** -19, "ragged": 2.0 ** -19, "upsampler": 2.0 ** -19,
         "conv_pre": 2.0 ** -16, "act_btc": 2.0 ** -15, "act_bct": 2.0 ** -15}

# ---- which kernel a float convolution with taps > 1 runs (gemm_conv.hip: dispatch_conv<float> / dispatch_narrow<float>) ------------
# KT = ceil(Cin / 16) k-steps, NT = ceil(N / 16) column tiles.  The narrow forms take Cin <= 64 and N <= 64 while the packed weights fit
# (taps NT KT KiB <= 150 KiB; the C = 96 clause needs (KT, NT) = (6, 6), which no narrow form is built for, so it falls through);
# conv_narrow_lds is compiled for 2-byte types only (`if constexpr (sizeof(T) == 2)`).  Inside that region: taps 3 / 7 / 11 with
# (KT, NT) = (1, 2) or (2, 3) -> conv_narrow_taps; otherwise (KT, NT) in NARROW_KN -> conv_narrow (so conv_narrow<f32,1,2> and <f32,2,3>
# are reached at any other tap count only); every other (KT, NT) and everything outside the region -> the tiled kernel, by N alone.
NARROW_KN = ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 3))
TAPS_KN = {(1, 2): (4, 4), (2, 3): (2, 4)}          # (KT, NT) -> (row tiles per wave TM, waves NW) of conv_narrow_taps
TILED = (("gemm_conv<f32,1,4,8,2,2,64>", 128), ("gemm_conv<f32,2,2,4,2,2,64,persist>", 64), ("gemm_conv<f32,2,2,4,3,2,64,persist>", 96),
         ("gemm_conv<f32,4,1,4,3,2,64>", 48), ("gemm_conv<f32,4,1,4,2,2,64>", 1))     # (form, N % this == 0), first match wins


def f32_conv_form(Cin, N, taps):
    """The form itts_gemm_conv launches for dtype fp32 and taps > 1: a function of (Cin, N, taps) alone."""
    assert taps > 1
    kt, nt = (Cin + KS32 - 1) // KS32, (N + 15) // 16
    if Cin <= 64 and N <= 64 and taps * nt * kt * 1024 <= 150 * 1024:
        if taps in (3, 7, 11) and (kt, nt) in TAPS_KN:
            return "conv_narrow_taps<f32,%d,%d,%d,%d,%d>" % ((kt, nt, taps) + TAPS_KN[(kt, nt)])
        if (kt, nt) in NARROW_KN:
            return f"conv_narrow<f32,{kt},{nt}>"
    return next(f for f, m in TILED if N % m == 0)


REACHABLE_F32_CONV = ({f"conv_narrow<f32,{kt},{nt}>" for kt, nt in NARROW_KN}
                      | {"conv_narrow_taps<f32,%d,%d,%d,%d,%d>" % (kn + (k,) + tn) for kn, tn in TAPS_KN.items() for k in (3, 7, 11)}
                      | {f for f, _ in TILED})


def row_tile(form):
    """BM, the output rows of one workgroup tile, from the template arguments in the form's name: conv_narrow 4 waves x 4 x 16 rows;
    conv_narrow_taps NW x TM x 16; gemm_conv<T,WM,WN,TM,...> 16 TM WM."""
    a = form[form.index("<") + 1:-1].split(",")[1:]
    if form.startswith("conv_narrow_taps"):
        return int(a[4]) * int(a[3]) * 16
    if form.startswith("conv_narrow<"):
        return 256
    assert form.startswith("gemm_conv<"), form
    return 16 * int(a[2]) * int(a[0])


# (Cin, N, [(k, d), ...]) per form.  Cin in {8, 24, 40}: the last k-step of 16 is half padding in each (itts_gemm_conv requires
# Cin % 8 == 0, so 8 of 16 columns is the only partial fp32 k-step there is), and KT = 1 / 2 / 3 takes the tiled kernel through its
# short-chunk path, one full chunk, and both; N = 1 (conv_post: the non-vector epilogue) and 20 (a
# partial column tile); (k, d) from the vocoder's {3, 7, 11} x {1, 3, 5}, with (11, 5) the widest halo it uses (50 rows) and (3, 32),
# (5, 16) at CV_MAX_HALO = 64; 5 and 9 taps where a form is reached at no vocoder tap count.  The first case of the list runs the controls.
KD = [(7, 3), (11, 5), (3, 1), (3, 32)]
KD_OTHER = [(5, 16), (9, 3), (2, 1)]
F32_CONV_CASES = (
    [(24, 24, KD), (24, 20, KD[:2]), (8, 16, KD), (16, 1, KD[:2]), (24, 1, [(7, 1), (3, 32)]), (48, 48, KD), (40, 48, KD[:2]),
     (16, 32, KD_OTHER), (8, 20, KD_OTHER[:2]), (32, 48, KD_OTHER), (24, 40, KD_OTHER[:2])]
    + [(C, N, [(k, d) for d in ((1, 3, 5, 32) if k == 3 else (1, 3, 5))]) for k in (3, 7, 11) for C, N in ((16, 32), (8, 20), (32, 48), (24, 40))]
    + [(24, 128, KD), (40, 256, KD[:2]), (8, 128, KD[:2]), (24, 64, KD), (40, 192, KD[:2]), (8, 64, KD[:2]), (96, 96, KD), (40, 96, KD[:2]),
       (8, 48, KD), (24, 144, KD[:2]), (40, 20, KD), (40, 1, KD[:2]), (8, 80, KD[:2])]
)
RAGGED_F32 = [(24, 24, 7, 3), (40, 64, 11, 5)]        # one narrow and one tiled form, lens [0, 1, tile - 1, tile, tile + 1, T]
RAGGED_T = 1100
# the six upsamplers of the vocoder: (Tn, cin, c, k, u); Tn <= 40 for the two widest; the narrowest stands first (it runs the control)
UPS = [(515, 48, 24, 4, 2), (37, 1536, 768, 8, 4), (40, 768, 384, 8, 4), (130, 384, 192, 4, 4), (257, 192, 96, 4, 4),
       (300, 96, 48, 4, 2)]
CONV_PRE = dict(B=3, T=129, C=1280, N=1536, k=7, d=1)
# the first case of each convolution family (it runs the controls): (C, N, k, d); T = the form's row tile + 1, B = 3, epilogue "bias"
FIRST_CONV = {"narrow": (24, 24, 7, 3), "narrow_taps": (24, 40, 7, 3), "tiled": (24, 128, 7, 3)}
CONTROL_EPIS = ("bias", "resid_acc_third")


def conv_seed(C, N, k, d, T):
    return 1000 + 13 * C + 7 * N + 101 * k + 3 * d + T


def ragged_lens(tile, T=RAGGED_T):
    return [0, 1, tile - 1, tile, tile + 1, T]


def conv_case(dtype, B, T, C, N, k, d, epi, seed, device="cpu"):
    """Seeded operands of one 'same' convolution (off0 = -(k-1)d/2) with the epilogue `epi`, drawn in float64 and rounded to their
    storage types: (x, w [k][C][N], bias, off0, rk) with rk the reference's keyword operands (resid, yprev, scale, bias2)."""
    x = rnd(B, T, C, seed=seed, device=device).to(dtype)
    w = (rnd(k, C, N, seed=seed + 1, device=device) / math.sqrt(C * k)).to(dtype)
    bias = (rnd(N, seed=seed + 2, device=device) * 0.1).float()
    has_r, acc, scale, has_b2 = EPIS[epi]
    rk = {}
    if has_r:
        rk["resid"] = rnd(B, T, N, seed=seed + 3, device=device).to(dtype)
    if acc:
        rk["yprev"] = rnd(B, T, N, seed=seed + 4, device=device).to(dtype)
    if scale != 1.0:
        rk["scale"] = scale
    if has_b2:
        rk["bias2"] = (rnd(B, N, seed=seed + 5, device=device) * 0.1).float()
    return x, w, bias, -((k - 1) * d // 2), rk


def ups_case(dtype, B, Tn, cin, c, k, u, seed, bias2, device="cpu"):
    """Operands of one up-sampler (ConvTranspose1d, stride u, as 1 or 2 taps over [Tn (+1) rows][u c columns]): (x, w [cin][c][k],
    bias [u c], bias2 [B][u c] or None)."""
    w = (rnd(cin, c, k, seed=seed, device=device) / math.sqrt(cin * k / u)).to(dtype)
    x = rnd(B, Tn, cin, seed=seed + 1, device=device).to(dtype)
    bias = (rnd(c, seed=seed + 2, device=device) * 0.1).float().repeat(u).contiguous()
    b2 = (rnd(B, u * c, seed=seed + 3, device=device) * 0.1).float() if bias2 else None
    return x, w, bias, b2


def convtr_taps(w, u):
    """ConvTranspose1d weight [Cin][Cout][k] (stride u, padding (k - u) / 2, k in {u, 2u}) as (taps [n][Cin][u Cout], off0, y_shift):
    t' + pad = q u + s,  y[t'] = x[q] W[:, :, s] + x[q - 1] W[:, :, s + u]  (the second term only when k = 2u)."""
    Cin, Cout, k = w.shape
    pad = (k - u) // 2
    if k == u:
        return w.permute(0, 2, 1).reshape(1, Cin, u * Cout).contiguous(), 0, -pad * Cout
    assert k == 2 * u
    lo = w[:, :, :u].permute(0, 2, 1).reshape(Cin, u * Cout)
    hi = w[:, :, u:].permute(0, 2, 1).reshape(Cin, u * Cout)
    return torch.stack([hi, lo], 0).contiguous(), -1, -pad * Cout


def x_through_fp16(x):
    """fp32-only control: x rounded to fp16 before the product (a 16-bit path taken by mistake)."""
    return x.to(F16).to(x.dtype)


def kpad_overrun(x, w):
    """fp32-only control: the K-padding columns of the last k-step (Cin = 24: columns 24..31) read as what follows the row in memory --
    x's next row, and on the weight side the next tap's first rows (zeros past the end of either operand): (x', w') with Cin rounded
    up to whole k-steps, for `conv_ref`.  The kernels guard those columns (col < Cin) and the packed weights are zero there."""
    B, T, Cin = x.shape
    taps, _, N = w.shape
    P = -Cin % KS32
    xf = torch.cat([x.double().reshape(B, T * Cin), torch.zeros(B, P, dtype=torch.float64, device=x.device)], 1)
    wf = torch.cat([w.double().reshape(taps * Cin, N), torch.zeros(P, N, dtype=torch.float64, device=w.device)], 0)
    return xf.unfold(1, Cin + P, Cin).contiguous(), wf.unfold(0, Cin + P, Cin).transpose(1, 2).contiguous()


def conv_controls(x, w, k, off0, d, T, bias, rk, eps, vr=None):
    """{description: wrong float64 reference} of the fp32 convolution controls on one case's operands; eps: the TAP32 of its family, or
    None to leave the perturbed tap out (TAP32 is fixed on the family's first case, epilogue "bias": an epilogue that adds |resid| and
    |y_prev| to S has a wider bound)."""
    N = w.shape[2]
    ref = lambda xx, ww: conv_ref(xx, ww, k, off0, d, T, bias=bias, vr=vr, **rk)[0]  # noqa: E731
    out = {"x rounded to fp16 before the product": ref(x_through_fp16(x), w)}
    if eps is not None:
        out[f"one weight tap off by 2^{int(math.log2(eps))} relative"] = ref(x, perturbed_tap(w, k // 2, eps))
    if T > 3:
        out["input shifted by one row at a tile boundary"] = ref(shifted_rows(x, min(T - 2, 128 if T > 200 else T // 2)), w)
    if N > 1:
        out["two output channels of a 16-channel block exchanged"] = ref(x, swapped_last(w))
    if x.shape[2] % KS32 and vr is None:
        out["the K-padding columns of the last k-step read past the row's end"] = ref(*kpad_overrun(x, w))
    return out


# ---- activation -----------------------------------------------------------------------------------------------------
AA_TT = {64: 56, 48: 76, 32: 120, 24: 160}      # AaTile<CS>::TT (aa_tile.h): output rows of one workgroup tile


def aa_cs(C):
    """Channel-slice width itts_aa_snake_fwd picks (layout 0)."""
    return 64 if C % 64 == 0 else 48 if C % 48 == 0 else 32 if C % 32 == 0 else 24


def act_lengths(C):
    TT = AA_TT[aa_cs(C)]
    return [1, 2, 5, 6, 7, TT - 1, TT, TT + 1, 2 * TT + 1]


ACT_C = (192, 384, 96, 32, 24, 128)             # CS = 64, 64, 48, 32, 24 and C = 128 (two 64-channel slices: grid.y = 2)
BCT_T = (1, 255, 256, 257)                      # aa_snake_bct<f32>: 256 outputs per workgroup
# the first case of each activation family (it runs the controls): (B, T, C)
FIRST_ACT = {"act_btc": (2, 2 * 56 + 1, 192), "act_bct": (2, 257, 48)}


def act_seed(T, C):
    return 7000 + 11 * C + T


def act_case(dtype, B, T, C, seed, xscale=1.0, al=None, be=None, device="cpu"):
    x = (rnd(B, T, C, seed=seed, device=device) * xscale).to(dtype)
    al = (rnd(C, seed=seed + 1, device=device) * 0.3).float() if al is None else al
    be = (rnd(C, seed=seed + 2, device=device) * 0.3).float() if be is None else be
    return x, al, be


def act_controls(x, al, be, up, dn, eps, lens=None):
    """{description: wrong float64 reference} of the fp32 activation controls (mfma=False); eps: the TAP32 of the family."""
    T = x.shape[1]
    TT = AA_TT[aa_cs(x.shape[2])]
    tb = TT if T > TT + 1 else T // 2
    ref = lambda *a, **kw: act_ref(*a, False, lens, **kw)[0]  # noqa: E731
    return {"input shifted by one row at a tile boundary": ref(shifted_rows(x, tb), al, be, up, dn),
            "zero padding at the sequence end": ref(x, al, be, up, dn, end_pad="zero"),
            f"one down-filter tap off by 2^{int(math.log2(eps))} relative": ref(x, al, be, up, perturbed_filter(dn, eps)),
            "alpha and beta swapped": ref(x, be, al, up, dn),
            "two channels of a 16-channel block exchanged": ref(swapped_last(x), al, be, up, dn)}


# ---- tanh_pcm -------------------------------------------------------------------------------------------------------
TANH32_MEASURED = 0.653 * 2.0 ** -24    # worst |tanhf(x) - tanh64(x)| on an MI355X over tanh_inputs of every size and input type
TANH32 = 2 * TANH32_MEASURED
TANH32_LOUD_MEASURED = 1.314 * 2.0 ** -24   # the same over tanh_loud_inputs (n = TANH_LOUD_N, every input type)
TANH32_LOUD = 2 * TANH32_LOUD_MEASURED
TANH_LOUD_N = 65536 + 257
PCM_SHARE = 0.01
TANH_GRID_CAP = 4096 * 256          # itts_tanh_pcm: at most 4096 workgroups of 256 threads; a larger n walks the stride loop
TANH_N = (1, 255, 257, TANH_GRID_CAP + 257)
TANH_SEED = 8100
# seeds at which the float64 reference alone keeps the share of PCM elements with a choice under PCM_SHARE (found by a search on the
# CPU, asserted by test_vocoder_refs_cpu.py); every other (n, type) takes TANH_SEED
TANH_SEEDS = {(255, F32): 8104, (255, F16): 8104, (257, F32): 8104, (257, F16): 8104}


def tanh_seed(n, dtype):
    return TANH_SEEDS.get((n, dtype), TANH_SEED)


BF16_FLOOR = 2.0 ** -8


def tanh_inputs(n, dtype, seed, apply_tanh, device="cpu"):
    """n inputs rounded to `dtype`: N(0, 0.05) in the main (a quiet waveform: 2 * 32767 * TANH32 alone is 0.51 % of the elements, so the
    1 % cap leaves room only where ulp_f32(v) is small), every 4096th element 300 times that, cut at |x| = 20, and the last one 20
    (tanhf saturates to +-1 from |x| ~ 9), and for apply_tanh = 0 (x is already a waveform) exactly +-1.0 (the clamp's own value) and
    values past +-1 (clamped).
    bf16 inputs are pushed away from zero by BF16_FLOOR = 2^-8.  A bf16 value below it is m 2^e with m < 256 and e >= -16 or so, so
    32768 x is an integer for a large part of them, 32767 tanh(x) = 32768 x - x - 32767 x^3 / 3 + ... lies |x| below that integer, and
    every such |x| < W = 32767 (ulp + TANH32) ~ 0.003 has a choice: 1.3 % of a million N(0, 0.05) inputs in the float64 reference alone,
    whatever the seed.  From 2^-8 on the distance |x| exceeds W.  (fp16 and fp32 inputs carry 11 and 24 bits: 32768 x is no integer
    there.)"""
    x = rnd(n, seed=seed, device=device) * 0.05
    if dtype == BF16:
        x = x + torch.sign(x) * BF16_FLOOR
    big = torch.arange(n, device=device) % 4096 == 7
    x = torch.where(big, torch.clamp(x * 300.0, -20.0, 20.0), x)
    if n > 1:
        x[-1] = 20.0
    if not apply_tanh:
        for i, v in enumerate((1.0, -1.0, 1.5, -3.0, 0.99999)):
            if 8 + 16 * i < n:
                x[8 + 16 * i] = v
    return x.to(dtype)


def tanh_loud_inputs(n, dtype, seed, device="cpu"):
    """The wav-only case that samples tanh where tanhf's error is largest: N(0, 1.5) cut at |x| = 20 -- more than four fifths of the elements
    in 0.3 <= |x| <= 9, the rest near zero or saturated.  Held to ulp_f32 + TANH32_LOUD; no PCM output is judged on it (at this level
    2 * 32767 * TANH32_LOUD alone passes the 1 % cap)."""
    return torch.clamp(rnd(n, seed=seed, device=device) * 1.5, -20.0, 20.0).to(dtype)


def tanh_ref(x, apply_tanh, t32=None):
    """(v64, wav bound): the float64 value of the waveform sample and the bound of the fp32 `wav` output (t32: TANH32 by default)."""
    if not apply_tanh:
        v = x.double()
        return v, torch.zeros_like(v)
    v = torch.tanh(x.double())
    return v, ulp(v, F32) + (TANH32 if t32 is None else t32)


def pcm_allowed(x, apply_tanh, gain=32767.0, rounding="trunc"):
    """(lo, hi) int64: the PCM values a sample may take (lo == hi where there is no choice).  gain / rounding: the negative controls
    (32768 in place of 32767; round to nearest in place of truncation)."""
    v, wb = tanh_ref(x, apply_tanh)
    rd = torch.trunc if rounding == "trunc" else torch.round
    if not apply_tanh:       # exact: one fp32 rounding of an exact product
        t = torch.clamp((gain * v).float().double(), -32767.0, 32767.0)
        p = rd(t).long()
        return p, p
    t, W = gain * v, gain * wb
    a, b = rd(torch.clamp(t - W, -32767.0, 32767.0)).long(), rd(torch.clamp(t + W, -32767.0, 32767.0)).long()
    return torch.minimum(a, b), torch.maximum(a, b)


def pcm_verdict(pcm, lo, hi):
    """(elements outside [lo, hi], share of elements with a choice): a PCM output passes iff the first is 0 and the share <= PCM_SHARE."""
    p = pcm.long()
    return int(((p < lo) | (p > hi)).sum()), float((lo != hi).double().mean())
