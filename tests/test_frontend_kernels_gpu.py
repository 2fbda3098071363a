"""fp64 parity of the prompt front-end kernel forms (csrc/frontend.hip: the conditioner's and the speaker encoder's kernels),
element by element, with bounds derived from where each form rounds -- the third counterpart of test_vocoder_kernels_gpu.py and
test_decode_kernels_gpu.py.

Every case generates its operands in float64, rounds them to the storage type, runs ONE HIP kernel on them and compares it with
the float64 reference of tests/frontend_refs.py on those rounded operands (the references, their bounds and the operand
generators live there, device-agnostic, so that tests/test_frontend_refs_cpu.py can hold them to torch's float64 operators and
prove on the CPU that every control below leaves its bound).  Assertions are per element, |y - ref| <= bound with `bound` a tensor
(fp64_check.check names the worst element).  Every 16-bit form runs in bf16 and f16.

For every case:
  * outputs are prefilled with a finite non-zero sentinel pattern (7 .. 11 by element index) and every element the header says is
    not written must keep it: rows past T / M of a packed tile, tiles outside [y_row0, y_row0 + M), the columns of a wider operand,
    and 64 elements behind every buffer.  itts_scale_resid is the one kernel that writes its operand's padding rows (it maps whole
    1-KiB blocks: padding rows of out = gate * padding rows of y + padding rows of res); include/indextts_hip.h says so per entry point.
  * every packed operand a kernel READS has the padding rows of its last tile filled with 1000, not zeros (frontend_refs.padded +
    pack_padded): a kernel that summed them (se_gate, col_stats) lands far outside its bound, and the first case of those families
    proves it with a control that sums them in the reference.
  * the bounds (frontend_refs, next to each reference): ulp_T(ref) for the store; (n + 1) 2^-24 S for a counted fp32 chain, 2^-21 S
    for MFMA / long fmaf chains; (|x| + 2) 2^-24 for __expf; Lipschitz constants SiLU 1.10, ReLU 1, sigmoid 1/4; a LayerNorm behind a
    computed value carries the input error through rstd |lw| plus the relative error of rstd; sqrt of a variance: the variance error
    over the two roots with the 1e-12 clamp.  fp32 outputs (itts_rows y, itts_se_gate) get no ulp_T term.
  * the one measured constant is C_ERF, the accuracy of the device library's erff (frontend_refs.C_ERF; test_geglu prints the
    measurement of its run as `fp64 | measure | ...`).
  * negative controls: the first case of a family at which the control can differ at all re-evaluates the assertion against a
    deliberately wrong reference; every one must fail; the kernel still runs once.  (res2_step: at T = dil + 1 every tap reflects and
    reversed taps are the same sum, and a `first` step has no previous chunk, so the controls sit on (17, 2, 7) and (45, 3, 1);
    glu_dwconv_ln_silu: at T = 1 there is no padding to get wrong, the controls sit on (9, 128, 15); mha_small: on the first case with
    a position term and more than one key; col_stats: on T = 17, where a divisor of T - 1 still moves a bf16 value.)

Every case's form key (tests/frontend_forms.py) is in PINNED, and `test_production_calls_are_pinned_forms` records the front-end
calls of the 2-layer conditioner engine (120 and 437 mel frames) and the speaker engine (57 and 600 frames) and requires every
call's key to be a pinned one.

Every check prints one line `fp64 | kind | case | worst err / bound`; profiles/frontend_kernels_fp64.txt is that output.
"""
import inspect

import pytest
import torch

import frontend_forms as forms
import frontend_refs as R
from fp64_check import bad, note, ok, tname, ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [BF16, F16]
TAIL = 64


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def sent(n, dtype):
    """n + TAIL sentinel elements 7 .. 11 by index (exact in bf16 / f16 / fp32); a kernel gets the first n."""
    return (torch.arange(n + TAIL, device=DEV) % 5 + 7).to(dtype)


def kept(buf, n, what):
    assert torch.equal(buf[n:], sent(n, buf.dtype)[n:]), f"{what}: elements behind the output were written"


def mtp_of(T):
    return (T + 15) // 16


def packed_in(x, mtp):
    """x [T][K] (storage type) as a packed operand of mtp row tiles whose padding rows hold 1000."""
    return R.pack_padded(R.padded(x, mtp))


def check_packed_out(buf, mtp, K, row0, rows, what):
    """Unpacks a packed output of mtp tiles written into a sentinel buffer: returns rows [row0, row0 + rows); every other row of
    every tile, and the tail behind the operand, must hold the sentinel."""
    n = mtp * 16 * K
    full = R.unpack_padded(buf[:n], mtp, K)
    want = R.unpack_padded(sent(n, buf.dtype)[:n], mtp, K)
    mask = torch.ones(mtp * 16, dtype=torch.bool, device=DEV)
    mask[row0:row0 + rows] = False
    assert torch.equal(full[mask], want[mask]), f"{what}: rows of the packed operand outside [{row0}, {row0 + rows}) were written"
    kept(buf, n, what)
    return full[row0:row0 + rows]


# ------------------------------------------------------------------------------------------------- subsample_conv
SUB_CASES = [(7, 20, 64), (3, 5, 8), (5, 9, 12), (5, 11, 1024), (4, 145, 8), (5, 131, 512), (41, 100, 512)]
SUB_KEYS = {  # what each case is there for (frontend_forms.subsample_conv: staged, 2nd channel pass, 2nd frequency pass, idle waves)
    (7, 20, 64): (True, False, False, False), (3, 5, 8): (False, False, False, False), (5, 9, 12): (False, False, False, True),
    (5, 11, 1024): (True, True, False, False), (4, 145, 8): (True, False, True, False), (5, 131, 512): (False, False, True, False),
    (41, 100, 512): (True, False, False, False)}
PINNED = {forms.subsample_conv(*c) for c in SUB_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", SUB_CASES, ids=str)
def test_subsample_conv_fp64(nat, dtype, case):
    """bias + nine fmafs, ReLU, one store: bound = ulp_T(ref) + 10 * 2^-24 S, S = |b| + sum |w| |mel|.  An even T leaves the last
    mel row unused: it holds 1000."""
    T, Fq, C = case
    assert forms.subsample_conv(T, Fq, C)[1:] == SUB_KEYS[case]
    mel, w, b = R.subsample_inputs(T, Fq, C, device=DEV)
    T2, F2 = (T - 3) // 2 + 1, (Fq - 3) // 2 + 1
    n = T2 * C * F2
    buf = sent(n, dtype)
    nat.subsample_conv(mel, w, b, buf[:n].view(T2, C * F2))
    what = f"subsample_conv {tname(dtype)} T={T} F={Fq} C={C}"
    kept(buf, n, what)
    got = buf[:n].view(T2, C * F2)
    ref, S = R.subsample_conv_ref(mel, w, b)
    bound = R.subsample_conv_bound(ref, S, dtype)
    ok(what, got, ref, bound)
    if case == SUB_CASES[0]:
        bad(what, "the stride-2 window shifted by one mel row", got, R.subsample_conv_ref(mel, w, b, row_shift=1)[0], bound)
        bz = b.clone()
        bz[-1] = 0
        bad(what, "the last channel's bias omitted", got, R.subsample_conv_ref(mel, w, bz)[0], bound)
        bad(what, "ReLU dropped", got, R.subsample_conv_ref(mel, w, b, relu=False)[0], bound)


# ------------------------------------------------------------------------------------------------- mha_small
# (Tq, Tk, H, rel, out_mtp (0 = ceil(Tq / 16)), extra row stride)
MHA_CASES = [(1, 1, 1, False, 0, 0), (16, 32, 1, True, 0, 0), (17, 33, 2, True, 0, 0), (5, 128, 1, False, 0, 0), (33, 129, 2, True, 0, 0),
             (32, 161, 2, False, 3, 40), (59, 59, 8, True, 0, 0), (32, 91, 8, False, 0, 0)]
PINNED |= {forms.mha_small(*c[:4]) for c in MHA_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", MHA_CASES, ids=str)
def test_mha_small_fp64(nat, dtype, case):
    """Form (a): the reference walks the kernel's 32-key steps (round-robin over four waves, a running maximum per wave), rounds
    q + u, q + v and P = exp(s - m_step) where the kernel does, sums the rounded P and merges the four states in float64.  Bound:
    ulp_T(ref) + sum_j [near_j ulp_T(P_j) + p_j delta_j] |v_j| / l + |ref| sum_j [near_j ulp_T(P_j) + p_j delta_j] / l with
    delta_j = 2^-21 (T_j + T_max) + 2^-19 and T_j = (sum |q+u| |k_j| + sum |q+v| |p_j|) scale (the position term included); the
    second sum is the same errors in the normaliser, which sums the rounded P here.  q, k and v are views of one buffer whose other
    columns hold 1000; rows past Tq of the output's last tile keep the sentinel (the kernel returns before the store)."""
    Tq, Tk, H, rel, out_mtp, extra = case
    d = H * 64
    q, k, v, pos, bu, bv = R.mha_inputs(Tq, Tk, H, rel, dtype, device=DEV)
    stride = 3 * d + extra
    src = torch.full((max(Tq, Tk), stride), R.POISON, dtype=dtype, device=DEV)
    src[:Tq, :d], src[:Tk, d:2 * d], src[:Tk, 2 * d:3 * d] = q.reshape(Tq, d), k.reshape(Tk, d), v.reshape(Tk, d)
    mtp = out_mtp or mtp_of(Tq)
    buf = sent(mtp * 16 * d, dtype)
    nat.mha_small(src, src[:, d:], src[:, 2 * d:], buf, Tq, Tk, H, stride, stride, stride, mtp, 0.125, pos=pos, bias_u=bu, bias_v=bv)
    what = f"mha_small {tname(dtype)} Tq={Tq} Tk={Tk} H={H} {'relpos' if rel else 'plain'}" + (f" out_mtp={mtp} stride={stride}" if extra else "")
    got = check_packed_out(buf, mtp, d, 0, Tq, what)
    ref, E, info = R.mha_small_ref(q, k, v, 0.125, pos, bu, bv)
    bound = R.mha_small_bound(ref, E, dtype)
    ok(what, got, ref, bound)
    r = (got.double() - ref).abs() / bound
    i = int(torch.argmax(r))
    note("detail", f"{what}: share of the midpoint allowance in the worst element's bound", (info["E_flip"].flatten()[i] / bound.flatten()[i]).item())
    if case == MHA_CASES[1]:
        for name, wrong in R.mha_controls(q, k, v, pos, bu, bv):
            bad(what, name, got, wrong, bound)


# ------------------------------------------------------------------------------------------------- glu_dwconv_ln_silu
# (T, C, taps, y_mtp, class): class None deals the |mean| / sigma classes by thirds of the rows; a case too short for that (the
# convolution blends all its rows) names the class of all its rows, and the 16-wave case, the one that fills red[16], runs in each
GLU_CASES = [(1, 128, 31, 1, 0), (9, 128, 15, 1, 0), (17, 256, 7, 3, None), (5, 2048, 15, 1, 0), (5, 2048, 15, 1, 1), (5, 2048, 15, 1, 2),
             (33, 512, 15, 3, None)]
GLU_CLASS = ("|mean| < sigma", "|mean| ~ 8 sigma", "|mean| > 64 sigma")
PINNED |= {forms.glu_dwconv_ln_silu(*c[:3]) for c in GLU_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", GLU_CASES, ids=lambda c: str(c[:4]) + (f"-class{c[4]}" if c[4] else ""))
def test_glu_dwconv_ln_silu_fp64(nat, dtype, case):
    """GLU (a / (1 + __expf(-g)): (|g| + 4) 2^-24 relative) -> a chain of `taps` fmafs on the bias ((taps + 1) 2^-24 S) -> LayerNorm
    behind that computed value (the error of c goes through the mean, d = c - mean, the variance and rstd |lw|) -> SiLU (L = 1.10 and
    its own (|v| + 4) 2^-24) -> one store; frontend_refs.glu_dwconv_ln_silu_ref spells the terms out.  By thirds of the rows the conv
    output has |mean| / sigma below 1, about 8 and above 64 where T / 3 > (taps - 1) / 2 (frontend_refs.glu_inputs); each third is
    reported on its own.  A shorter case has one class in all its rows; the 16-wave case, whose block sums fill red[16], runs in all
    three.  One row has one outlier channel of 60 sigma (frontend_refs.glu_outlier_row).  Rows past T of the packed output keep the sentinel (grid = T rows)."""
    T, C, taps, mtp, cls = case
    x, w, b, lw, lb = R.glu_inputs(T, C, taps, dtype, cls, device=DEV)
    buf = sent(mtp * 16 * C, dtype)
    nat.glu_dwconv_ln_silu(x, w, b, lw, lb, buf, T, C, mtp)
    what = f"glu_dwconv_ln_silu {tname(dtype)} T={T} C={C} taps={taps} y_mtp={mtp}" + (f" all rows {GLU_CLASS[cls]}" if cls is not None else "")
    got = check_packed_out(buf, mtp, C, 0, T, what)
    ref, bound = R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, dtype=dtype)
    ok(what, got, ref, bound)
    if cls is None:
        third = torch.clamp(torch.arange(T, device=DEV) * 3 // T, max=2)[:, None]
        for i, name in enumerate(GLU_CLASS):
            ok(f"{what} rows with {name}", got, ref, bound, third == i)
    if case == GLU_CASES[1]:
        f = lambda **kw: R.glu_dwconv_ln_silu_ref(x, w, b, lw, lb, **kw)[0]  # noqa: E731
        bad(what, "the first tap dropped", got, f(drop_tap=0), bound)
        bad(what, "padding replicated from the edge rows instead of zero", got, f(replicate=True), bound)
        bad(what, "the value and gate halves exchanged", got, f(swap_halves=True), bound)
        bad(what, "variance over C - 1", got, f(var_div=C - 1), bound)


# ------------------------------------------------------------------------------------------------- rows
P = lambda **kw: kw  # noqa: E731
# (M, D, nslab, options): x / bias default to present; out: "y" (fp32 alone), "alias" (y = x), "packed" (copy alone), "both";
# row0 / mtp: where the packed copy goes; special: "zero" (an all-zero row), "fold" (fold_rows rows), ctl: the controls that run here
ROWS_CASES = [
    (37, 1280, 9, P(ctl=("slab", "bias"))),
    (37, 4, 9, P()), (37, 512, 9, P()), (37, 1024, 9, P()), (37, 1028, 9, P()), (37, 2048, 9, P()),          # the D edges at nslab 9
    (37, 1280, 0, P()), (37, 1280, 1, P()), (37, 1280, 8, P()), (37, 1280, 32, P()), (37, 1280, 64, P()),    # the nslab edges at D 1280
    (37, 1280, 9, P(norm=1, ctl=("mean",))), (37, 1280, 9, P(norm=2, ctl=("sqrtd",))),
    (37, 512, 9, P(norm=1, out="both")), (37, 2048, 9, P(norm=2, out="both")),
    (37, 512, 0, P(norm=1, bias=False, out="alias", packed=True)),                                           # the conditioner's final LayerNorm
    (37, 1280, 0, P(bias=False, out="packed")),
    (37, 512, 64, P(x=False, out="both", row0=32, mtp=5)), (37, 512, 32, P(x=False, out="both", row0=32, mtp=5)),   # embed.out's slabs
    (37, 1280, 0, P(bias=False, out="both", mtp=3)),                                                         # the latents into [latents ; context]
    (37, 1280, 0, P(norm=2, bias=False, special="zero")),                                                    # the Perceiver's final norm
    (37, 1280, 0, P(norm=1, bias=False, special="fold")), (37, 512, 9, P(norm=1, special="fold", out="both")),
    (1, 4, 9, P()), (1, 2048, 64, P(norm=1)), (1, 1280, 0, P(bias=False, out="packed")), (1, 1024, 1, P(norm=2, out="both")),
]


def rows_key(M, D, nslab, o):
    out = o.get("out", "y")
    return forms.rows(M, D, o.get("x", True), o.get("bias", True), nslab, o.get("norm", 0), out != "packed",
                      out in ("packed", "both") or o.get("packed", False))


PINNED |= {rows_key(*c) for c in ROWS_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", range(len(ROWS_CASES)), ids=lambda i: "%d-M%d-D%d-s%d" % ((i,) + ROWS_CASES[i][:3]))
def test_rows_fp64(nat, dtype, case):
    """The fp32 y against the count-based bound, no ulp term: the sum is x, the bias and nslab slabs in fixed order, (nslab + 2) 2^-24 S;
    then the norm's terms (frontend_refs.rows_ref: the error of the mean, of d = v - mean, of the variance, of rstd; for norm 2 of
    |v|^2 and its root).  The packed copy is bit-equal to the rounded fp32 row the kernel wrote (where there is no fp32 output it is
    held to the same bound plus ulp_T); only rows [y_row0, y_row0 + M) of its operand are written.  An all-zero row under norm 2
    comes out as zeros, not NaN."""
    M, D, nslab, o = ROWS_CASES[case]
    norm, out, special = o.get("norm", 0), o.get("out", "y"), o.get("special")
    x, slab, bias, w, b = R.rows_inputs(M, D, nslab, norm, x=o.get("x", True), bias=o.get("bias", True), special=special, device=DEV)
    what = f"rows {tname(dtype)} M={M} D={D} nslab={nslab} norm={norm} {'x' if x is not None else '-'}{'b' if bias is not None else '-'} " \
           f"out={out}" + (f" {special}" if special else "")
    want_packed = out in ("packed", "both") or o.get("packed", False)
    row0, mtp = o.get("row0", 0), o.get("mtp", mtp_of(M))
    ybuf = sent(M * D, torch.float32)
    y = None if out == "packed" else (x if out == "alias" else ybuf[:M * D].view(M, D))
    x0 = x.clone() if x is not None else None
    pbuf = sent(mtp * 16 * D, dtype) if want_packed else None
    nat.rows(M, D, dtype, x=x, slab=slab, nslab=nslab, bias=bias, norm=norm, w=w, b=b, y=y, y_packed=pbuf, y_row0=row0, y_mtp=mtp)
    ref, bound = R.rows_ref(M, D, x0, slab, bias, norm, w, b)
    if y is not None:
        if out != "alias":
            kept(ybuf, M * D, what)
        ok(what + ": y", y, ref, bound)
        if special == "fold":
            for cls, cname in enumerate(("|mean| = 0", "|mean| = 8 sigma", "|mean| = 64 sigma", "one outlier feature")):
                rows_ = (torch.arange(M, device=DEV) % 4 == cls)[:, None]
                if rows_.any():
                    ok(f"{what}: y rows with {cname}", y, ref, bound, rows_)
        if special == "zero":
            assert (y[M // 2] == 0).all(), f"{what}: the all-zero row is not zeros"
    if want_packed:
        gp = check_packed_out(pbuf, mtp, D, row0, M, what)
        if y is not None:
            assert torch.equal(gp, y.to(dtype)), f"{what}: the packed copy is not the rounded fp32 row"
        else:
            ok(what + ": packed copy", gp, ref, bound + ulp(ref, dtype))
    for c in o.get("ctl", ()):
        kw = dict(slab=dict(drop_slab=8), bias=dict(bias_twice=True), mean=dict(no_mean=True), sqrtd=dict(no_sqrt_d=True))[c]
        name = dict(slab="slab 8 (the first of the second pass) dropped", bias="the bias added twice", mean="LayerNorm without the mean",
                    sqrtd="sqrt(D) dropped")[c]
        bad(what, name, y, R.rows_ref(M, D, x0, slab, bias, norm, w, b, **kw)[0], bound)


def test_rows_refusals(nat):
    x = torch.zeros(37, 2052, device=DEV)
    y = torch.zeros(37, 2052, device=DEV)
    with pytest.raises(nat.NativeError):
        nat.rows(37, 2052, BF16, x=x, y=y)                                        # D > 2048
    with pytest.raises(nat.NativeError):
        nat.rows(37, 6, BF16, x=x, y=y)                                           # D % 4 != 0
    yp = torch.zeros(3 * 16 * 64, dtype=BF16, device=DEV)
    with pytest.raises(nat.NativeError):
        nat.rows(37, 64, BF16, x=x, y_packed=yp, y_row0=16, y_mtp=3)              # rows [16, 53) do not fit three tiles
    assert (yp == 0).all() and (y == 0).all()


# ------------------------------------------------------------------------------------------------- geglu
GEGLU_CASES = [(1, 32, 0), (17, 96, 3), (32, 3424, 0)]
PINNED |= {forms.geglu(*c) for c in GEGLU_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", GEGLU_CASES, ids=str)
def test_geglu_fp64(nat, dtype, case):
    """0.5 g (1 + erff(g / sqrt 2)) x: bound = ulp_T(ref) + (C_ERF + 1) 2^-24 0.5 |g x| + 4 * 2^-24 |ref| -- erff's absolute error and
    the rounding of its argument both enter 1 + erf absolutely, which the cancellation tail (gate < -5) keeps; one addition and
    three products follow.  C_ERF is the one measured constant (frontend_refs.C_ERF): the first case measures the device erff
    (torch.erf on fp32 runs the same device-library function) over the gate grid and prints it."""
    M, Kp, y_mtp = case
    mtp = y_mtp or mtp_of(M)
    h = R.geglu_inputs(M, Kp, dtype, device=DEV)
    buf = sent(mtp * 16 * Kp, dtype)
    nat.geglu(h, buf, M, Kp, y_mtp)
    what = f"geglu {tname(dtype)} M={M} Kp={Kp} y_mtp={mtp}"
    got = check_packed_out(buf, mtp, Kp, 0, M, what)
    ref, bound = R.geglu_ref(h, dtype)
    ok(what, got, ref, bound)
    if case == GEGLU_CASES[0]:
        a = R.geglu_inputs(32, 3424, dtype, seed=0, device=DEV)[:, 3424:].float() * 0.70710678118654752
        meas = ((torch.erf(a).double() - torch.erf(a.double())).abs().max() / R.U).item()
        note("measure", f"erff {tname(dtype)} gate grid: worst |erff - erf| in units of 2^-24 (C_ERF = {R.C_ERF})", meas)
        bad(what, "the halves exchanged", got, R.geglu_ref(h, swap_halves=True)[0], bound)
        cut = ref.clone()
        cut[:, -4:] = R.SENT
        bad(what, "the last 4-column group of a row missing", got, cut, bound)


# ------------------------------------------------------------------------------------------------- im2col_reflect
# (T, F, taps, dil, Kp, mtp)
IM2COL_CASES = [(3, 5, 5, 1, 32, 1), (7, 100, 5, 1, 512, 1), (9, 8, 7, 2, 64, 2), (10, 12, 3, 3, 64, 1), (5, 32, 3, 1, 96, 1)]
PINNED |= {forms.im2col_reflect(*c[:5]) for c in IM2COL_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", IM2COL_CASES, ids=str)
def test_im2col_reflect_exact(nat, dtype, case):
    """A gather and one rounding: equal to the rounded reference bit for bit -- the bound is a quarter of the storage grid's spacing,
    which no two distinct values of the type are within.  T = pad + 1 is the deepest reflection; rows past T keep the sentinel."""
    T, Fq, taps, dil, Kp, mtp = case
    x = R.im2col_inputs(T, Fq, device=DEV)
    buf = sent(mtp * 16 * Kp, dtype)
    nat.im2col_reflect(x, buf, taps, dil, Kp, mtp)
    what = f"im2col_reflect {tname(dtype)} T={T} F={Fq} taps={taps} dil={dil} Kp={Kp} mtp={mtp}"
    got = check_packed_out(buf, mtp, Kp, 0, T, what)
    tiny = 0.25 * ulp(R.im2col_reflect_ref(x, taps, dil, Kp).to(dtype).double(), dtype)
    rounded = lambda mode: R.im2col_reflect_ref(x, taps, dil, Kp, mode).to(dtype).double()  # noqa: E731
    ok(what, got, rounded("reflect"), tiny)
    if case == IM2COL_CASES[0]:
        bad(what, "replicate instead of reflect", got, rounded("replicate"), tiny)
        bad(what, "symmetric reflection that includes the edge", got, rounded("symmetric"), tiny)
        with pytest.raises(nat.NativeError):
            nat.im2col_reflect(x[:2].contiguous(), buf, taps, dil, Kp, mtp)      # T <= pad


# ------------------------------------------------------------------------------------------------- res2_step
# (T, dil, chunk, first, mtp, controls)
CAT_PAD = 500.0   # the padding rows of cat, unlike y1's 1000: a write there shows
RES2_CASES = [(2, 1, 1, True, 1, False), (5, 4, 2, False, 1, False), (17, 2, 7, False, 2, True), (45, 3, 1, True, 4, True),
              (45, 3, 4, False, 3, False)]
PINNED |= {forms.res2_step(c[0], c[4], c[2], c[1], c[3]) for c in RES2_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", RES2_CASES, ids=str)
def test_res2_step_fp64(nat, dtype, case):
    """Six chained 32-deep MFMAs + bias -> ReLU -> one fmaf (BatchNorm) -> one store: bound = ulp_T(ref) + |scale| (2^-21 S +
    2^-24 |pre|) + 2^-24 |ref|; the reference rounds y1 + cat where the kernel does.  Every other element of cat -- the other
    chunks, the padding rows -- is untouched; chunk 0 is copied bit for bit when `first`, rows < T only.  The padding rows hold 1000
    in y1 and 500 in cat: they are never read (rows are clamped to T - 1 before the reflection) and never written, so a copy or a
    store without its `t < T` guard would put y1's 1000, or a computed value, where cat must still hold 500."""
    T, dil, s, first, mtp, controls = case
    C = 512
    y1, cat, w, b, sc, sh = R.res2_inputs(T, dtype, device=DEV)
    wp = nat.pack_weight(w.permute(2, 1, 0).reshape(192, 64).contiguous())
    y1p, catp = packed_in(y1, mtp), R.pack_padded(R.padded(cat, mtp, CAT_PAD))
    nat.res2_step(y1p, catp, wp, b, sc, sh, T, mtp, s, dil, first)
    what = f"res2_step {tname(dtype)} T={T} dil={dil} chunk={s} first={first} mtp={mtp}"
    after = R.unpack_padded(catp, mtp, C)
    want = R.padded(cat, mtp, CAT_PAD)
    want[:T, 64 * s:64 * s + 64] = after[:T, 64 * s:64 * s + 64]
    if first:
        want[:T, :64] = y1[:, :64]
    assert torch.equal(after, want), f"{what}: cat changed outside chunk {s}" + (" / chunk 0 is not y1's" if first else "")
    got = after[:T, 64 * s:64 * s + 64]
    a = (y1, cat, w, b, sc, sh, s, dil, first, dtype)
    ref, bound = R.res2_step_ref(*a)
    ok(what, got, ref, bound)
    if controls:
        bad(what, "replicate padding", got, R.res2_step_ref(*a, mode="replicate")[0], bound)
        bad(what, "taps reversed", got, R.res2_step_ref(*a, reverse_taps=True)[0], bound)
        bad(what, "BatchNorm shift omitted", got, R.res2_step_ref(*a, no_shift=True)[0], bound)
        if not first:
            bad(what, "the previous chunk not added", got, R.res2_step_ref(*a, add_prev=False)[0], bound)


# ------------------------------------------------------------------------------------------------- se_gate
SE_CASES = [(1, 64, 16), (64, 128, 32), (77, 512, 128), (37, 1024, 512)]
PINNED |= {forms.se_gate(*c, mtp_of(c[0])) for c in SE_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", SE_CASES, ids=str)
def test_se_gate_fp64(nat, dtype, case):
    """fp32 output, no ulp term: the mean is mtp additions per lane, four shuffle steps and a division ((mtp + 6) 2^-24 sum |y| / T),
    each product a long fmaf chain (2^-21 S) that carries the error in front of it, ReLU L = 1, sigmoid L = 1/4 plus its own
    (|x| + 4) 2^-24.  The padding rows of y hold 1000: the guard `(mt + j) * 16 + r < Tn` is what keeps them out."""
    T, C, H = case
    mtp = mtp_of(T)
    y, w1, b1, w2, b2 = R.se_inputs(T, C, H, dtype, device=DEV)
    buf = sent(C, torch.float32)
    nat.se_gate(packed_in(y, mtp), w1, b1, w2, b2, buf, T, C, H, mtp)
    what = f"se_gate {tname(dtype)} T={T} C={C} H={H}"
    kept(buf, C, what)
    ref, bound = R.se_gate_ref(y, w1, b1, w2, b2, mtp)
    ok(what, buf[:C], ref, bound)
    if case == SE_CASES[0]:
        f = lambda **kw: R.se_gate_ref(y, w1, b1, w2, b2, mtp, **kw)[0]  # noqa: E731
        bad(what, "the mean over mtp * 16 rows (the padding rows summed)", buf[:C], f(rows=R.padded(y, mtp)), bound)
        bad(what, "b1 omitted", buf[:C], f(no_b1=True), bound)
        bad(what, "ReLU dropped", buf[:C], f(relu=False), bound)


# ------------------------------------------------------------------------------------------------- scale_resid
SR_CASES = [(1, 32, 1), (40, 96, 3), (77, 512, 5)]
PINNED |= {forms.scale_resid(*c) for c in SR_CASES}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", SR_CASES, ids=str)
def test_scale_resid_fp64(nat, dtype, case):
    """One fmaf and one store: bound = ulp_T(ref) + 2^-24 |ref|.  The kernel maps whole 1-KiB blocks, so the padding rows of out
    ARE written: gate * (padding row of y) + (padding row of res) -- the reference covers all mtp * 16 rows.  (77, 512, 5) writes the
    middle third of a [T][3 C] operand whose outer thirds keep the sentinel."""
    T, C, mtp = case
    y, res, gate = R.scale_resid_inputs(T, C, dtype, device=DEV)
    y, res = R.padded(y, mtp), R.padded(res, mtp, 500.0)
    wide = 3 if C == 512 else 1
    n = mtp * 16 * C
    buf = sent(wide * n, dtype)
    off = n if wide == 3 else 0
    nat.scale_resid(R.pack_padded(y), R.pack_padded(res), gate, buf[off:], T, C, mtp)
    what = f"scale_resid {tname(dtype)} T={T} C={C} mtp={mtp}" + (" into the middle third of [T][3 C]" if wide == 3 else "")
    kept(buf, wide * n, what)
    if wide == 3:
        assert torch.equal(buf[:n], sent(wide * n, dtype)[:n]) and torch.equal(buf[2 * n:3 * n], sent(wide * n, dtype)[2 * n:3 * n]), \
            f"{what}: the outer thirds were written"
    got = R.unpack_padded(buf[off:off + n], mtp, C)
    ref, bound = R.scale_resid_ref(y, res, gate, dtype)
    ok(what, got, ref, bound)
    if case == SR_CASES[0]:
        bad(what, "the gate shifted by 8 channels", got, R.scale_resid_ref(y, res, gate, dtype, gate_shift=8)[0], bound)


# ------------------------------------------------------------------------------------------------- col_stats
CS_T = [1, 16, 17, 77, 512, 513, 1000]
PINNED |= {forms.col_stats(T, 64, mtp_of(T), wtd, wtd) for T in CS_T for wtd in (False, True)}


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("T", CS_T)
def test_col_stats_fp64(nat, dtype, T, C, weighted):
    """T = 512 is the last one-pass size, 513 the first multi-pass one, 1000 takes two full passes; C = 64 / 128: one and two
    workgroups.  Bound (frontend_refs.col_stats_ref): a sum is at most n = ceil(mtp / 8) + 12 additions, a weight carries
    (|l - max| + 2) 2^-24 of __expf; the mean's error enters d = x - m and with it the variance, whose error goes over the two roots
    (the kernel's being at least 1e-6 behind the 1e-12 clamp: the constant channel 3 sits on it); the affine map scales it; one store.
    The padding rows of x hold 1000: the guards `t < Tn` / `row_of(mb, j) < Tn` are what keeps them out.  Logits are flat in every
    fourth channel and put most weight on a few frames in the others."""
    mtp = mtp_of(T)
    x, logit, sc, sh = R.col_stats_inputs(T, C, dtype, device=DEV)
    buf = sent(2 * C, dtype)
    kw = dict(logit=logit, scale=sc, shift=sh) if weighted else {}
    nat.col_stats(packed_in(x, mtp), buf, T, C, mtp, **kw)
    what = f"col_stats {tname(dtype)} T={T} C={C} {'softmax-weighted + affine' if weighted else 'plain'}"
    kept(buf, 2 * C, what)
    args = (logit, sc, sh) if weighted else ()
    ref, bound = R.col_stats_ref(x, mtp, dtype, *args)
    ok(what, buf[:2 * C], ref, bound)
    if T == 17 and C == 64:
        if weighted:
            bad(what, "uniform weights", buf[:2 * C], R.col_stats_ref(x, mtp, dtype, *args, uniform=True)[0], bound)
            bad(what, "shift[C + c] taken from shift[c]", buf[:2 * C], R.col_stats_ref(x, mtp, dtype, *args, shift_low=True)[0], bound)
        else:
            bad(what, "statistics over the padded rows", buf[:2 * C], R.col_stats_ref(R.padded(x, mtp), mtp, dtype)[0], bound)
            bad(what, "variance over T - 1", buf[:2 * C], R.col_stats_ref(x, mtp, dtype, var_div_t1=True)[0], bound)


# ------------------------------------------------------------------------------------------------- production forms
def test_production_calls_are_pinned_forms(nat, monkeypatch):
    """The front-end calls of the 2-layer conditioner engine at 120 and 437 mel frames and of the speaker engine at 57 and 600
    frames, recorded through the module attributes the engines call: every call's form key is one a case above pins."""
    from test_frontend_gpu import _cond_model, _vocoder
    import synth
    seen = []

    def wrap(name, key_of):
        """Records key_of(arguments of the call as _native's own signature binds them, defaults applied), then makes the call."""
        real = getattr(nat, name)
        sig = inspect.signature(real)

        def rec(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            seen.append(key_of(bound.arguments))
            return real(*a, **kw)
        monkeypatch.setattr(nat, name, rec)

    has = lambda a, n: a[n] is not None  # noqa: E731
    wrap("subsample_conv", lambda a: forms.subsample_conv(a["mel"].shape[0], a["mel"].shape[1], a["w"].shape[0]))
    wrap("mha_small", lambda a: forms.mha_small(a["Tq"], a["Tk"], a["H"], has(a, "pos")))
    wrap("glu_dwconv_ln_silu", lambda a: forms.glu_dwconv_ln_silu(a["T"], a["Cn"], a["w"].shape[1]))
    wrap("rows", lambda a: forms.rows(a["M"], a["D"], has(a, "x"), has(a, "bias"), a["nslab"], a["norm"], has(a, "y"), has(a, "y_packed")))
    wrap("geglu", lambda a: forms.geglu(a["M"], a["Kp"], a["y_mtp"]))
    wrap("im2col_reflect", lambda a: forms.im2col_reflect(a["x"].shape[0], a["x"].shape[1], a["taps"], a["dil"], a["Kp"]))
    wrap("res2_step", lambda a: forms.res2_step(a["T"], a["mtp"], a["chunk"], a["dil"], a["first"]))
    wrap("se_gate", lambda a: forms.se_gate(a["T"], a["Cn"], a["H"], a["mtp"]))
    wrap("scale_resid", lambda a: forms.scale_resid(a["T"], a["Cn"], a["mtp"]))
    wrap("col_stats", lambda a: forms.col_stats(a["T"], a["Cn"], a["mtp"], has(a, "logit"), has(a, "scale")))
    m = _cond_model(BF16)
    for frames in (120, 437):
        mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, frames), -6.0, 2.0)).to(DEV)
        assert torch.isfinite(m.get_conditioning(mel, None)).all()
    n_cond = len(seen)
    v = _vocoder(F16)
    for frames in (57, 600):
        mel = torch.from_numpy(synth.uniform("in.ref_mel", (1, frames, 100), -6.0, 2.0)).to(DEV)
        assert torch.isfinite(v.speaker_embedding(mel)).all()
    torch.cuda.synchronize()
    assert n_cond >= 2 * 12 and len(seen) - n_cond >= 2 * 30, (n_cond, len(seen))
    for key in sorted(set(seen), key=str):
        print(f"production | {key} | {seen.count(key)} calls | {'pinned' if key in PINNED else 'NOT PINNED'}")
    missing = sorted({k for k in seen if k not in PINNED}, key=str)
    assert not missing, f"production calls whose form no case pins: {missing}"
