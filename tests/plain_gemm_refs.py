"""float64 reference of itts_gemm_conv at taps = 1 (csrc/gemm_conv.hip: gemm_plain_kernel and the tiled convolution kernel with
HALO = 0 or one tap), its per-element error bounds, the negative controls, the operand generator and the case lists of
tests/test_plain_gemm_kernels_gpu.py.  Device-agnostic plain torch: every function works on the device of its operands and makes no
call into the library, so tests/test_plain_gemm_refs_cpu.py can hold the reference to torch's own float64 operators and prove that
every control leaves its bound, without a GPU.

Reference, as include/indextts_hip.h states the operation (operands as the kernel sees them: x and w rounded to the storage type,
bias / bias2 fp32, resid and the previous y in the output's type; `scale` as its fp32 value):
      v = scale * (act(x w + bias + bias2) + resid)          y = (accumulate ? y_prev : 0) + v
      S = |scale| (sum_k |x w| + |bias| + |bias2| + |resid|) + |y_prev|
With split-K slab s is the product over columns [(s KT) / ks * KS, ((s + 1) KT) / ks * KS) alone (KT = K / KS k-steps of KS = 32
columns, 16 at fp32), held to its own S.

Bounds, per element (the project's own: docstring of tests/test_decode_kernels_gpu.py; u = 2^-24):
      T output                       ulp_T(ref) + 2^-21 S
      fp32 output                    2^-21 S                  (slabs, y_f32, every output of the fp32 dtype)
      gelu_new, T output             ulp_T(ref) + 1.13 * 2^-21 S + 2^-21 |ref|
      gelu_new, fp32 output          1.13 * 2^-21 S + G32,    G32 = [(14 |a| + 3) |gelu(p)| + 5.5 |p|] u
  with p the pre-activation and a = sqrt(2 / pi) (p + 0.044715 p^3).  1.13 is the Lipschitz constant of gelu_new (the error of p
  goes through it).  G32 is the activation's own fp32 error, which a 16-bit store hides and an fp32 store does not; it is derived
  from the kernel's chain (csrc/common.h, gelu_new), not measured:
      a    = k * (p + c * p * p * p)       three products, one sum and one product, the terms of the sum of one sign (no
                                           cancellation), k and c rounded to fp32 (half an ulp each): |da| <= 6 u |a|
      e    = __expf(2 a)                   one product with log2 e and the hardware exp2: (|2 a| + 2) u relative (the decode file's
                                           figure), and exp carries da: 2 |a| * 6 u.  Together  de = (14 |a| + 2) u  relative
      q    = __fdividef(2, 1 + e)          the sum u, the hardware reciprocal one ulp = 2 u, a rounding of the product u: 4 u
                                           relative; de enters as de e / (1 + e), and q e / (1 + e) = g / (1 + e) <= g with
                                           g = 1 + tanh = 2 e / (1 + e) the exact factor:
                                           |dq| <= g de + 4 u q <= g de + 8 u      (q <= 2)
      th   = 1 - q,  g' = 1 + th           u |th| <= u and u g <= 2 u.  For a negative argument q -> 2 and g = 2 - q CANCELS: the
                                           absolute error of q stays while g shrinks -- that is the 11 u below, absolute in g
                                           |dg| <= g de + 11 u
      y    = 0.5 p g'                      one rounding (0.5 p is exact): |dy| <= 0.5 |p| (g de + 11 u) + u |y| = |y| (de + u) + 5.5 u |p|
  Checked on the CPU (test_plain_gemm_refs_cpu.py): the same chain evaluated in numpy float32 (`gelu_chain_f32`, __expf as
  exp2(x * log2 e) in float32) on the fp32 gelu cases' own float64 pre-activations, against float64 gelu_new -- the emulation's worst
  error is EMU_G32 of G32 (at p = -3.18, where the cancellation term is nearly all of G32), and twice that must fit.  The figure is in
  profiles/plain_gemm_fp64.txt as well.

Negative controls (CONTROLS): each re-evaluates the reference with one thing wrong; the kernel's output is compared with it under
the same bound and must fail."""
import numpy as np
import torch

import plain_forms as forms
from fp64_check import rnd, ulp

U = 2.0 ** -24          # unit roundoff of fp32
CHAIN = 2.0 ** -21      # the project's fp32-chain figure (MFMA chains), relative to the magnitude sum
L_GELU = 1.13           # Lipschitz constant of gelu_new
EMU_G32 = 0.269         # worst |gelu_chain_f32 - gelu_new| / G32 over the fp32 gelu cases (test_gelu_f32_term_holds_twice_the_emulation)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TAG = {BF16: "bf16", F16: "f16", F32: "f32"}
K_GELU, C_GELU = 0.7978845608028654, 0.044715

CONTROLS = {
    "rowshift": "x shifted by one row from row 128 on",
    "swap_wtiles": "the first two 16-column weight tiles exchanged",
    "drop_last_kstep": "the last k-step (the last 8 columns of a partial one) left out",
    "slice_boundary": "every inner slice boundary one k-step late",
    "no_resid": "resid left out",
    "bias_rot4": "bias rotated by 4 columns",
    "scale_before_resid": "scale applied before the residual",
    "no_prev": "the previous y not added",
}


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(K_GELU * (x + C_GELU * x ** 3)))


def gelu_chain_f32(p):
    """The kernel's gelu_new chain (csrc/common.h) step by step in numpy float32; p: float32 array."""
    f = np.float32
    with np.errstate(over="ignore"):
        a = f(K_GELU) * (p + f(C_GELU) * p * p * p)
        e = np.exp2((f(2.0) * a) * f(1.4426950408889634))          # __expf(x) = exp2(x * log2 e)
        th = f(1.0) - f(2.0) / (f(1.0) + e)                         # __fdividef
        return f(0.5) * p * (f(1.0) + th)


def gelu_f32_term(pre):
    """G32 of the module docstring."""
    a = K_GELU * (pre + C_GELU * pre ** 3)
    return ((14.0 * a.abs() + 3.0) * gelu_new(pre).abs() + 5.5 * pre.abs()) * U


# ----------------------------------------------------------------------------------------------------------- cases
class Case:
    """One launch: y [B][M][N] (split-K: slabs [ks][M][N]) = itts_gemm_conv(taps 1) of x [B][M][K], w [K][N].
    resid: None, "own" (a buffer of its own) or "alias" (resid = y, in place); dts: the dtypes the case runs in."""

    def __init__(self, fam, M, N, K, B=1, ks=1, bias=True, bias2=False, act=0, y_f32=False, resid=None, acc=False, scale=1.0,
                 ctl=(), dts=(BF16, F16)):
        self.fam, self.M, self.N, self.K, self.B, self.ks = fam, M, N, K, B, ks
        self.bias, self.bias2, self.act, self.y_f32, self.resid, self.acc, self.scale = bias, bias2, act, y_f32, resid, acc, scale
        self.ctl, self.dts = tuple(ctl), tuple(dts)

    @property
    def kind(self):
        """The epilogue kind: what the epilogue reads and what it writes."""
        if self.ks > 1:
            return "slab"
        parts = [n for n, on in (("bias", self.bias), ("bias2", self.bias2), ("gelu", self.act), ("resid=" + str(self.resid), self.resid),
                                 ("scale", self.scale != 1.0), ("acc", self.acc)) if on]
        return "+".join(parts or ["store"]) + ("->f32" if self.y_f32 else "->T")

    def at(self, cus):
        """The case with a row count that depends on the part (M = "wide": the first 128 x 160 row count, less 57 rows)."""
        if self.M != "wide":
            return self
        c = Case(self.fam, forms.first_wide_mblocks(self.N, cus) * 128 - 57, self.N, self.K, self.B, self.ks, self.bias, self.bias2,
                 self.act, self.y_f32, self.resid, self.acc, self.scale, self.ctl, self.dts)
        return c

    def out_dtype(self, dtype):
        return F32 if (self.y_f32 or self.ks > 1 or dtype == F32) else dtype

    def seed(self):
        return (self.M * 1000003 + self.N * 10007 + self.K * 101 + self.B * 7 + self.ks) % (2 ** 31 - 1)

    def __str__(self):
        return (f"{self.fam} M={self.M} N={self.N} K={self.K}" + (f" B={self.B}" if self.B > 1 else "") + (f" ks={self.ks}" if self.ks > 1 else "")
                + f" {self.kind}")


EPI = dict(M=300, N=256, K=160)
CASES = (
    # M edges at one tile column and one chunk.  M = 300 stands first: the row-shift control needs rows behind row 128
    [Case("m-edge", 300, 128, 128, ctl=("rowshift", "swap_wtiles", "drop_last_kstep", "bias_rot4"))]
    + [Case("m-edge", M, 128, 128) for M in (1, 127, 128, 129)]
    # K edges: KT = 1 .. 5 (every path through the prologue, chunk tails of 1 - 3 steps), a partial k-step, 1280 + 32, FC2's depth
    + [Case("k-edge", 129, 256, K, ctl=("drop_last_kstep", "swap_wtiles") if K in (32, 40, 160) else ()) for K in (32, 64, 96, 128, 160, 40, 1312, 5120)]
    # tile order: 5 and 9 m-blocks under GM = 4 and 8 (one full and one partial L2 patch), 15 and 27 workgroups
    + [Case("tile-order", 600, 384, 64, ctl=("rowshift", "swap_wtiles")), Case("tile-order", 1100, 384, 1664)]
    # epilogues: the production kinds, then the remaining documented ones, then the scalar path (N % 4 != 0)
    + [Case("epilogue", **EPI, ctl=("bias_rot4", "rowshift")),
       Case("epilogue", **EPI, act=1, ctl=("bias_rot4",)),
       Case("epilogue", **EPI, y_f32=True, resid="alias", ctl=("no_resid",)),
       Case("epilogue", **EPI, resid="own", ctl=("no_resid",)),
       Case("epilogue", **EPI, resid="own", scale=1.0 / 3.0, acc=True, ctl=("scale_before_resid", "no_prev", "no_resid")),
       Case("epilogue", **EPI, bias2=True, ctl=("bias_rot4",)),
       Case("epilogue", **EPI, y_f32=True),
       Case("epilogue", 300, 1282, 160, resid="own", ctl=("no_resid", "bias_rot4"))]
    # split-K into fp32 slabs
    + [Case("split-k", 129, 128, 1280, ks=2, bias=False, ctl=("slice_boundary", "drop_last_kstep", "swap_wtiles")),
       Case("split-k", 300, 1280, 1280, ks=3, bias=False, ctl=("slice_boundary", "rowshift")),
       Case("split-k", 129, 128, 128, ks=4, bias=False),
       Case("split-k", 300, 128, 2048, ks=64, bias=False, ctl=("slice_boundary",)),
       Case("split-k", 129, 1280, 5120, ks=3, bias=False)]
    # the 128 x 160 form (row count by the round rule) and the same N at a row count that takes 128 x 128
    + [Case("wide", "wide", 640, 96, act=1, ctl=("rowshift", "swap_wtiles", "drop_last_kstep")),
       Case("wide", "wide", 640, 96),
       Case("wide", 300, 640, 96)]
    # N % 64 == 0: either side of rows * (N / 64) >= 448
    + [Case("n64", 300, 192, 96, B=3, ctl=("rowshift", "swap_wtiles", "drop_last_kstep"), dts=(BF16, F16, F32)),
       Case("n64", 70, 192, 96, B=150, dts=(BF16, F16, F32))]
    # the convolution forms a plain GEMM falls through to: N % 96, N % 48, the rest
    + [Case("fall-through", 129, N, 128, dts=(BF16, F16, F32)) for N in (96, 144, 80)]
    # fp32 (KS = 16): KT = 1, 3, 5, 80
    + [Case("fp32", M, 128, K, dts=(F32,), **kw) for K in (16, 48, 80, 1280) for M in (129, 300)
       for kw in (dict(ctl=("drop_last_kstep", "swap_wtiles", "bias_rot4") if (K, M) == (16, 129) else ()), dict(act=1),
                  dict(resid="alias", ctl=("no_resid",) if (K, M) == (16, 129) else ()))]
    + [Case("fp32", "wide", 640, 96, dts=(F32,))]
)


# ----------------------------------------------------------------------------------------------------------- operands
def operands(c, dtype, device="cpu"):
    """Seeded operands of case c, drawn in float64 and rounded to their storage types: dict of x [B][M][K], w [K][N] (dtype), bias [N],
    bias2 [B][N] (fp32), resid, y_prev [B][M][N] (the output's type) -- None where the case has none."""
    s, yt = c.seed(), c.out_dtype(dtype)
    o = dict(x=rnd(c.B, c.M, c.K, seed=s, device=device).to(dtype), w=rnd(c.K, c.N, seed=s + 1, scale=c.K ** -0.5, device=device).to(dtype),
             bias=None, bias2=None, resid=None, y_prev=None)
    if c.bias:
        o["bias"] = rnd(c.N, seed=s + 2, scale=0.1, device=device).float()
    if c.bias2:
        o["bias2"] = rnd(c.B, c.N, seed=s + 3, scale=0.1, device=device).float()
    if c.resid:
        o["resid"] = rnd(c.B, c.M, c.N, seed=s + 4, scale=2.0, device=device).to(yt)
    if c.acc:
        o["y_prev"] = rnd(c.B, c.M, c.N, seed=s + 5, device=device).to(yt)
    return o


# ----------------------------------------------------------------------------------------------------------- reference
def slices(c, dtype, shift=0):
    """Column ranges [k0, k1) of the ks slices (one range without split-K).  shift: inner boundaries `shift` k-steps late."""
    if c.ks <= 1:
        return [(0, c.K)]
    KS = forms.kstep(TAG[dtype])
    KT = c.K // KS
    cut = lambda s: 0 if s == 0 else KT if s == c.ks else forms.slice_ksteps(KT, c.ks, s)[0] + shift  # noqa: E731
    return [(cut(s) * KS, cut(s + 1) * KS) for s in range(c.ks)]


def plain_ref(c, dtype, o, ctl=None):
    """(ref, S, pre) float64 [B or ks][M][N] of case c on operands o; ctl: one of CONTROLS, evaluated wrong in that one way."""
    assert ctl is None or ctl in CONTROLS
    xd, wd = o["x"].double(), o["w"].double()
    KS = forms.kstep(TAG[dtype])
    if ctl == "rowshift":
        assert c.M >= 130
        xd = torch.cat([xd[:, :128], torch.roll(xd[:, 128:], -1, dims=1)], 1)
    if ctl == "swap_wtiles":
        wd = torch.cat([wd[:, 16:32], wd[:, :16], wd[:, 32:]], 1)
    accs, mags = [], []
    for k0, k1 in slices(c, dtype, shift=1 if ctl == "slice_boundary" else 0):
        if ctl == "drop_last_kstep":
            k1 -= KS if (k1 - k0) % KS == 0 else 8
        accs.append(xd[:, :, k0:k1] @ wd[k0:k1])
        mags.append(xd[:, :, k0:k1].abs() @ wd[k0:k1].abs())
    pre, S = (torch.cat(accs, 0), torch.cat(mags, 0)) if c.ks > 1 else (accs[0], mags[0])
    if o["bias"] is not None:
        b = o["bias"].double()
        if ctl == "bias_rot4":
            b = torch.roll(b, 4)
        pre, S = pre + b, S + b.abs()
    if o["bias2"] is not None:
        pre, S = pre + o["bias2"].double()[:, None, :], S + o["bias2"].double().abs()[:, None, :]
    v = gelu_new(pre) if c.act else pre
    sc = float(torch.tensor(c.scale, dtype=torch.float32))
    if o["resid"] is not None and ctl != "no_resid":
        r = o["resid"].double()
        v, S = (sc * v + r, sc * S + r.abs()) if ctl == "scale_before_resid" else (sc * (v + r), abs(sc) * (S + r.abs()))
    else:
        v, S = sc * v, abs(sc) * S
    if o["y_prev"] is not None:
        S = S + o["y_prev"].double().abs()
        if ctl != "no_prev":
            v = v + o["y_prev"].double()
    return v, S, pre


def bound(c, dtype, ref, S, pre):
    """The per-element bound of the module docstring for case c run in `dtype`."""
    yt = c.out_dtype(dtype)
    b = CHAIN * S * (L_GELU if c.act else 1.0)
    if yt != F32:      # a 16-bit output (PREC also lists fp32, for the fp32 pins: this bound keeps its own fp32 arm)
        b = b + ulp(ref, yt)
        if c.act:
            b = b + CHAIN * ref.abs()
    elif c.act:
        b = b + gelu_f32_term(pre)
    return b
