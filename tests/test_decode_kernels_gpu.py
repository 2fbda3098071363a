"""fp64 parity of the 16-bit decode-step kernel forms (skinny GEMM, decode attention, prefill attention), element by element,
with bounds derived from where each form rounds -- the GPT half's counterpart of test_vocoder_kernels_gpu.py.

Every case generates its operands in float64, rounds them to the storage type, runs one HIP kernel on them and compares it
with a float64 evaluation of the same operation on those rounded operands, on the GPU (explicit masks and sums, torch float64
matmul; no call into the library under test).  Assertions are per element, |y - ref| <= bound with `bound` a tensor
(fp64_check.check names the worst element).  Every case runs in bf16 and f16.

Skinny GEMM.  `form_key` turns nat.skinny_plan into (MT, SPW, NTB, FOLD, MAXW), the template arguments launch_skinny_mt
instantiates; each case asserts the key it was built for and adds it to PINNED, and `test_skinny_every_plannable_form_is_pinned`
holds PINNED against the list of every instantiation plan_skinny can ask for (see REACHABLE).
  Every form accumulates exact 16-bit products in fp32 and rounds once:
      T output:      |y - ref| <= ulp_T(ref) + 2^-21 S        S = sum_k |x w| + |bias| (+ |resid|)
      fp32 output:   |y - ref| <= 2^-21 S                     (STORE_F32, SLAB_F32 -- each slab against its own K slice --, RESID_F32's yf)
      activation f:  |y - ref| <= ulp_T(ref) + L 2^-21 S + 2^-21 |ref|
  (2^-21: the vocoder file's measured fp32-chain figure.)  L is the Lipschitz constant of the epilogue's function:
  gelu_new 1.13 (its derivative peaks at 1.129 near x = 1.5), SiLU 1.10 (derivative peaks at 1.0998 near x = 2.4), ReLU 1 and
  tanh 1 (the affine map behind the ReLU multiplies the pre-activation bound by |post_scale|).
  LayerNorm folded into the GEMM: the kernel computes rstd (h W' - mean c) + d with mean = S1 / K, var = max(S2 / K - mean^2, 0)
  from fp32 sums; the reference is the same formula in float64 on the rounded h, W' and the given c, d, and
      bound = ulp_T(ref) + 2^-21 [rstd (sum |h W'| + |mean| |c|) + |d|] + delta_r |ref - d|,
      delta_r = 2^-22 (E[h^2] + eps) / (var + eps)            (relative error of rstd: the fp32 cancellation in S2 / K - mean^2)
  Rows with |mean| / sigma of 0, 8 and 64 and a row with one outlier feature are in every folded case (see `fold_rows`).

Decode attention.  With p_j the softmax weights of the visible keys and A = sum_j p_j |v_j|:
      bound = ulp_T(ref) + C_ATTN A,   C_ATTN = 2^-16.
  fp32-level budget (u = 2^-24): a score is 8 fmaf per lane and 3 shuffle additions, |ds| <= 11 u sum |q k| / 8 (about 10 for these
  inputs: 110 u); __expf is one product with log2 e (|x| u, |x| <= 17 for any weight that matters) and the hardware exp2 (2 u):
  19 u; the sums l and o take at most 32 additions per lane and 6 merge steps, 40 u (the factors exp(m - M) of a merge multiply
  l and o alike and cancel in o / l).  Per weight about 170 u relative, and |out - ref| <= sum p_j d_j |v_j - out| <= 2 * 170 u A
  = 2^-15.6 A if every rounding pushed the same way.  That worst case is 1.3 x the cap of 2^-16 the bound may not exceed
  (1/16 of an f16 half-ulp); the roundings are independent, their sum grows with the square root of the counts (about 30 u A),
  so the cap stands and the measured ratios (profiles/decode_kernels_fp64.txt) say how far below it the kernel sits.
  Inputs put weight on the boundary keys: scores have a standard deviation of 2, and the first visible key, the key in front
  of it, the key at *pos and the first key of every quarter pass are given a score near the row's maximum, so a dropped or
  admitted boundary key moves the output far outside the bound.

Prefill attention (form (a) of the two the design allows).  The kernel rounds P = exp(s - m) to the storage type before P V while
the row sum uses the unrounded values.  The reference walks the same 64-key tiles from sequence position 0 with the running
maximum and rounds P where the kernel does.  What is left is the fp32 level, per weight: a score is two chained 32-deep MFMAs,
|ds_j| <= 2^-21 T_j with T_j = sum_d |q_d k_jd| / 8 (the fp32-chain figure of the GEMM bound), the running maximum is such a
score too (T_max), and __expf, the row sums and the normalisation add 2^-19 (19 u + 13 u); so the kernel's P_j sits within
      delta_j = 2^-21 (T_j + T_max) + 2^-19
  relative of the float64 P_j, and
      bound = ulp_T(ref) + sum_j [near_j ulp_T(P_j) + p_j delta_j] |v_j| / l + |ref| sum_j p_j delta_j
  (near_j: P_j lies within delta_j P_j of a rounding midpoint, the kernel may round it the other way; the last term: the same
  errors in the normaliser).  With scores of standard deviation 2 (4 at f16) T_j is 10-30 and delta_j reaches 2^-16.
  Two left-padded cases sit close to the bound by construction, not by accident: bf16 S = 130 pad 70 at 0.975 (query 100, 31 keys)
  and f16 S = 130 pad 5 at 0.815 (query 119).  In both, one heavy weight lies INSIDE the midpoint window -- P = 0.32324 at 8.6e-8
  relative from a bf16 midpoint (key 100, |v| = 1.55), P = 0.35535 at 2.5e-7 from an f16 one (key 112) -- and the kernel's fp32 P
  rounds the other way.  That costs ulp_T(P) |v| / l = 1.05e-3, and the allowance of exactly that amount is 98 % of the element's
  bound (ulp_T(ref) = 1.5e-5 there): a flip uses its own allowance up, whatever the seed, and a row without one sits far lower
  (every other case <= 0.58).  The fp32-level terms play no part (the ratio was the same under a flat 2^-16 A).
  Form (b) -- an exact reference with r_P A in the bound, r_P = 2^-9 (bf16) / 2^-12 (f16) -- was measured as well and a correct
  kernel does not meet it: one weight's rounding error reaches 2^-8 / 2^-11 relative at the bottom of a binade, and a query with two
  or three visible keys has nothing to average it over (bf16, prefix length 1, query 1: err 3.6e-3 against a bound of 2.8e-3, 1.29 x;
  f16, S = 130, pad 70: 1.02 x).  At f16 the left-padded cases scale q so that the scores spread over about 24 > 14 ln 2: subnormal
  and flushed-to-zero P occur and are rounded by the reference as well.

Negative controls: the first case of every family evaluates the same assertion against a reference that is wrong in one small
way (listed at each family); every one must fail.  The controls only re-evaluate the reference; the kernel runs once.

Every check prints one line `fp64 | kind | case | worst err / bound`; profiles/decode_kernels_fp64.txt is that output.
"""
import math

import numpy as np
import pytest
import torch

from fp64_check import bad, check, fold_rows, must_fail, note, ok, tname, ulp, walk_start, walk_step  # noqa: F401
from skinny_forms import GEMM_SHAPES, REACHABLE, form_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [BF16, F16]
PINNED = set()          # (dtype, form key) of every skinny-GEMM case that has run
KS = 32                 # k-step of the 16-bit MFMA forms
TAB = 64                # ITTS_KV_TAB: entries of a row's block table
C_ATTN = 2.0 ** -16


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------- skinny GEMM
def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


ACT = {"store": (lambda v: v, None), "gelu": (gelu_new, 1.13), "silu": (lambda v: v * torch.sigmoid(v), 1.10)}


def gemm_pre(x, w, bias, fold=None, kstat=None):
    """fp64 pre-activation of the GEMM and its bound ingredients: (pre, S, extra) with the fp32-level budget 2^-21 S + extra.
    fold = (c, d, eps): rstd (x w - mean c) + d with the row statistics over the first `kstat` columns (all of them by default)."""
    xd, wd = x.double(), w.double()
    acc, mag = xd @ wd, xd.abs() @ wd.abs()
    if fold is None:
        if bias is not None:
            acc, mag = acc + bias.double(), mag + bias.double().abs()
        return acc, mag, torch.zeros_like(acc)
    c, d, eps = fold
    xs = xd if kstat is None else xd[:, :kstat]
    mean = xs.mean(1, keepdim=True)
    m2 = (xs * xs).mean(1, keepdim=True)
    var = torch.clamp(m2 - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = rstd * (acc - mean * c.double()) + d.double()
    S = rstd * (mag + mean.abs() * c.double().abs()) + d.double().abs()
    delta_r = 2.0 ** -22 * (m2 + eps) / (var + eps)
    return pre, S, delta_r * (pre - d.double()).abs()


def run_gemm(nat, dtype, M, N, K, key, epi="store", ksplit=1, rpw=0, wide=False, fold=False, ypk=False, y_row0=0, copy=True,
             bs=0, controls=False, seed=0, pin=True):
    """One itts_gemm_skinny launch against the fp64 reference; asserts the form key; packed and row-major x give equal bits."""
    k = form_key(nat, dtype, M, N, K, ksplit, rpw, wide, fold)
    assert k == key, f"M={M} N={N} K={K} ksplit={ksplit} rows_per_wg={rpw} wide={wide} fold={fold}: planned {k}, case built for {key}"
    if pin:
        PINNED.add((dtype, k))
        if M > 96 and rpw == 0:      # the entry point chunks the rows: the last chunk plans for its own row count
            PINNED.add((dtype, form_key(nat, dtype, M - 96 * ((M - 1) // 96), N, K, ksplit, rpw, wide, fold)))
    what = f"gemm {tname(dtype)} {k} M={M} N={N} K={K} {epi}" + (f" ksplit={ksplit}" if ksplit > 1 else "") + \
        (f" rows_per_wg={rpw}" if rpw else "") + (" packed-y" if ypk else "") + (f" paged{bs}" if bs else "")
    x = (fold_rows(M, K, seed, DEV) if fold else rnd(M, K, seed=seed)).to(dtype)
    w = (rnd(K, N, seed=seed + 1) / math.sqrt(K)).to(dtype)
    bias = rnd(N, seed=seed + 2).float()
    bias[-1] = 0.75
    fo = None
    kw = dict(ksplit=ksplit, rows_per_wg=rpw, wide_wg=wide)
    if fold:
        fo = (w.double().sum(0).float().contiguous(), bias, 1e-5)
        kw.update(ln_c=fo[0], ln_eps=1e-5)
    wp = nat.pack_weight(w)
    mtp = (M + 15) // 16
    xp = nat.pack_activation(x)
    lim = lambda ref, S, extra, L=None: (ulp(ref, dtype) + (L or 1.0) * (2.0 ** -21 * S + extra) + (2.0 ** -21 * ref.abs() if L else 0.0))  # noqa: E731
    f32lim = lambda S, extra: 2.0 ** -21 * S + extra + 1e-300  # noqa: E731  (an empty K slice: exact zeros, a zero bound)

    def launch(xa, packed, **out):
        nat.gemm_skinny(dtype, M, N, K, wp, bias, x=xa, x_packed=packed, **kw, **out)

    def both(make_out, **out_kw):
        """Run with the row-major and the packed operand into fresh outputs; equal bits; returns the first's outputs."""
        o1, o2 = make_out(), make_out()
        launch(x, False, **{n: t for n, t in zip(out_kw["names"], o1)}, **out_kw["kw"])
        launch(xp, True, **{n: t for n, t in zip(out_kw["names"], o2)}, **out_kw["kw"])
        for a, b in zip(o1, o2):
            assert torch.equal(a, b), f"{what}: packed and row-major x differ"
        return o1

    refs = []      # (name, got, reference function of (x, w, bias, fold, kstat) -> ref, bound or None when re-evaluated)

    if epi in ACT or epi in ("relu_affine", "relu_affine_tanh"):
        post = None
        if epi in ACT:
            f, L = ACT[epi]
            code = {"store": nat.EPI_STORE, "gelu": nat.EPI_GELU_STORE, "silu": nat.EPI_SILU_STORE}[epi]
        else:
            sc, sh = (1.0 + 0.3 * rnd(N, seed=seed + 5)).float(), (0.3 * rnd(N, seed=seed + 6)).float()
            post, L = (sc, sh), 1.0
            code = nat.EPI_RELU_AFFINE_TANH_STORE if epi.endswith("tanh") else nat.EPI_RELU_AFFINE_STORE

            def f(v):
                r = torch.relu(v) * sc.double() + sh.double()
                return torch.tanh(r) if epi.endswith("tanh") else r
        ymtp = mtp + y_row0 // 16 + (1 if y_row0 else 0)
        mk = (lambda: (torch.full((ymtp * 16 * N,), 7.0, dtype=dtype, device=DEV),)) if ypk else \
            (lambda: (torch.full((M, N), 7.0, dtype=dtype, device=DEV),))
        okw = dict(epi=code, y_packed=ypk, post=post)
        if ypk and y_row0:
            okw.update(y_row0=y_row0, y_mtp=ymtp)
        (y,) = both(mk, names=("y",), kw=okw)
        if ypk:
            full = nat.unpack_activation(y, ymtp * 16, N)
            got = full[y_row0:y_row0 + M]
            rest = torch.cat([full[:y_row0], full[y_row0 + M:]])
            assert (rest == 7.0).all(), f"{what}: rows of the packed operand outside [y_row0, y_row0 + M) were written"
        else:
            got = y

        def ref_of(x_, w_, b_, fo_, kstat=None):
            pre, S, extra = gemm_pre(x_, w_, b_, fo_, kstat)
            r = f(pre)
            sc_ = post[0].double().abs() if post else 1.0
            return r, lim(r, S * sc_ + (post[1].double().abs() if post else 0.0), extra * sc_, L)
        refs.append(("y", got, ref_of))
    elif epi == "store_f32":
        (yf,) = both(lambda: (torch.full((M, N), 7.0, device=DEV),), names=("yf",), kw=dict(epi=nat.EPI_STORE_F32))

        def ref_of(x_, w_, b_, fo_, kstat=None):
            pre, S, extra = gemm_pre(x_, w_, b_, fo_, kstat)
            return pre, f32lim(S, extra)
        refs.append(("yf", yf, ref_of))
    elif epi == "resid":
        h0 = rnd(M, N, seed=seed + 3, scale=2.0).float()
        ymtp = mtp + y_row0 // 16 + (1 if y_row0 else 0)
        names = ("yf", "y") if copy else ("yf",)

        def mk():
            ycopy = torch.full((ymtp * 16 * N,) if ypk else (M, N), 7.0, dtype=dtype, device=DEV)
            return (h0.clone(), ycopy) if copy else (h0.clone(),)
        okw = dict(epi=nat.EPI_RESID_F32, y_packed=ypk and copy)
        if ypk and copy and y_row0:
            okw.update(y_row0=y_row0, y_mtp=ymtp)
        outs = both(mk, names=names, kw=okw)
        yf = outs[0]
        if copy:      # the T copy is the rounded new row, bit for bit
            full = nat.unpack_activation(outs[1], ymtp * 16, N) if ypk else outs[1]
            assert torch.equal(full[y_row0:y_row0 + M], yf.to(dtype)), f"{what}: the T copy is not the rounded fp32 row"
            if ypk:
                assert (torch.cat([full[:y_row0], full[y_row0 + M:]]) == 7.0).all(), f"{what}: rows outside the copy were written"

        def ref_of(x_, w_, b_, fo_, kstat=None):
            pre, S, extra = gemm_pre(x_, w_, b_, fo_, kstat)
            return pre + h0.double(), f32lim(S + h0.double().abs(), extra)
        refs.append(("yf", yf, ref_of))
    elif epi == "slab":
        (slab,) = both(lambda: (torch.full((ksplit, M, N), 7.0, device=DEV),), names=("yf",), kw=dict(epi=nat.EPI_SLAB_F32))
        sb = -(-(K // KS) // ksplit) * KS                 # k-steps are split evenly, the last slice takes the remainder

        def ref_of(x_, w_, b_, fo_, kstat=None):
            rs, bs_ = [], []
            for i in range(ksplit):
                pre, S, _ = gemm_pre(x_[:, i * sb:(i + 1) * sb], w_[i * sb:(i + 1) * sb], b_ if i == 0 else None)
                rs.append(pre)
                bs_.append(f32lim(S, 0.0))
            return torch.stack(rs), torch.stack(bs_)
        refs.append(("slab", slab, ref_of))
    elif epi == "qkv":
        H = N // 192
        D = H * 64
        pos = 37
        posd = i32([pos])
        if bs:
            e = (pos // bs) % TAB
            tab = np.zeros((M, TAB), dtype=np.int32)      # unmapped entries name the scratch block 0
            blocks = np.random.default_rng(seed).permutation(np.arange(1, 1 + 3 * M)).reshape(M, 3)
            for j in range(3):
                tab[:, (e - 1 + j) % TAB] = blocks[:, j]
            tab_d = i32(tab)
            mk = lambda: (torch.full((M, D), 7.0, dtype=dtype, device=DEV),  # noqa: E731
                          torch.full((1 + 3 * M, H, bs, 64), 7.0, dtype=dtype, device=DEV),
                          torch.full((1 + 3 * M, H, bs, 64), 7.0, dtype=dtype, device=DEV))
            okw = dict(epi=nat.EPI_QKV_CACHE, pos=posd, heads=H, smax=0, kv_tab=tab_d, kv_bs=bs)
        else:
            smax = 48
            mk = lambda: (torch.full((M, D), 7.0, dtype=dtype, device=DEV),  # noqa: E731
                          torch.full((M, H, smax, 64), 7.0, dtype=dtype, device=DEV),
                          torch.full((M, H, smax, 64), 7.0, dtype=dtype, device=DEV))
            okw = dict(epi=nat.EPI_QKV_CACHE, pos=posd, heads=H, smax=smax)
        q, kc, vc = both(mk, names=("y", "kcache", "vcache"), kw=okw)

        def appended(cache, entry_off=0):
            if bs:
                blk = torch.from_numpy(tab[:, (e + entry_off) % TAB].astype(np.int64)).to(DEV)
                return cache[blk, :, pos % bs].reshape(M, D)
            return cache[:, :, pos].reshape(M, D)
        for cache in (kc, vc):                            # nothing but position *pos of each row's own block was touched
            t = cache.clone()
            if bs:
                t[torch.from_numpy(tab[:, e].astype(np.int64)).to(DEV), :, pos % bs] = 7.0
            else:
                t[:, :, pos] = 7.0
            assert (t == 7.0).all(), f"{what}: a cache position other than *pos was written"
        got = torch.cat([q, appended(kc), appended(vc)], 1)

        def ref_of(x_, w_, b_, fo_, kstat=None):
            pre, S, extra = gemm_pre(x_, w_, b_, fo_, kstat)
            return pre, lim(pre, S, extra)
        refs.append(("q|k|v", got, ref_of))
        if controls and bs:
            r, b_ = ref_of(x, w, bias, fo)
            bad(what, "the append placed one block entry off", torch.cat([q, appended(kc, 1), appended(vc, 1)], 1), r, b_)
    else:
        raise AssertionError(epi)

    for name, got, ref_of in refs:
        ref, bound = ref_of(x, w, bias, fo)
        ok(f"{what} {name}", got, ref, bound)
        if fold:      # each class of rows (fold_rows) is reported and asserted on its own: the worst row must not hide the others
            for cls, cname in enumerate(("|mean| = 0", "|mean| = 8 sigma", "|mean| = 64 sigma", "one outlier feature")):
                rows_ = (torch.arange(M, device=DEV) % 4 == cls)[:, None]
                if rows_.any():
                    ok(f"{what} {name} rows with {cname}", got, ref, bound, rows_)
        if not controls:
            continue
        wz = w.clone()
        wz[K - KS:] = 0
        bad(what, "the last k-step of the last wave dropped", got, ref_of(x, wz, bias, fo)[0], bound)
        ws, bsw = w.clone(), bias.clone()
        ws[:, [1, 2]], bsw[[1, 2]] = w[:, [2, 1]], bias[[2, 1]]
        fs = fo
        if fold:
            cs = fo[0].clone()
            cs[[1, 2]] = fo[0][[2, 1]]
            fs = (cs, bsw, fo[2])
        bad(what, "two output columns of a 16-column tile exchanged", got, ref_of(x, ws, bsw, fs)[0], bound)
        bz = bias.clone()
        bz[-1] = 0
        bad(what, "the bias of the last column omitted", got, ref_of(x, w, bz, None if fo is None else (fo[0], bz, fo[2]))[0], bound)
        if M > 16:
            xs = x.clone()
            xs[[0, 16]] = x[[16, 0]]
            bad(what, "rows 0 and 16 of x exchanged", got, ref_of(xs, w, bias, fo)[0], bound)
        if fold:
            bad(what, "c off by 2^-9 relative", got, ref_of(x, w, bias, ((fo[0].double() * (1 + 2.0 ** -9)), bias, fo[2]))[0], bound)
            bad(what, "statistics over K - 32 columns", got, ref_of(x, w, bias, fo, K - KS)[0], bound)


# (M, N, K, key, options): chosen so that PINNED covers REACHABLE and the risks are on the table --
#   M one below / at / one above 16, 32, 64, 96 (MT 4 with an empty fourth tile, MT 6 with an empty sixth), M > 96 with rows_per_wg 16 / 32
#   and without (the entry point chunks the rows); N % 16 != 0 and N % 4 != 0 (50; 8194, the head); K = 96 (3 waves: the epilogue's
#   second unit loop), K = 1184 (37 k-steps: the last wave gets 2 of 5), K = 1408 (44: the last wave gets 2 of 6; the LoRA bank's
#   1280 + 128), K = 2720 (85: two register passes, the last wave gets 8 of 11), K = 5248 (164: three passes; 5120 + 128).
P = lambda **kw: kw  # noqa: E731
GEMM_CASES = [
    # ---- plain, MT 1
    (1, 50, 96, (1, 5, 1, False, 8), P(controls=True)),
    (15, 50, 1184, (1, 5, 1, False, 8), P(epi="gelu")),
    (16, 64, 1280, (1, 5, 1, False, 8), P(epi="silu", ypk=True)),
    (16, 64, 320, (1, 5, 1, False, 8), P(epi="relu_affine")),
    (9, 64, 320, (1, 5, 1, False, 8), P(epi="relu_affine_tanh")),
    (16, 4112, 1184, (1, 5, 2, False, 8), P(epi="store_f32")),
    (7, 8194, 160, (1, 5, 3, False, 8), P()),
    (16, 50, 1408, (1, 10, 1, False, 8), P()),
    (3, 50, 2720, (1, 10, 1, False, 8), P(epi="gelu")),
    (5, 8194, 5248, (1, 10, 2, False, 8), P()),
    (16, 4112, 1408, (1, 10, 2, False, 8), P(epi="resid")),
    (1, 64, 2720, (1, 10, 1, False, 16), P(wide=True, epi="resid", ypk=True)),
    (13, 50, 5248, (1, 10, 1, False, 16), P(wide=True)),
    (13, 384, 1280, (1, 5, 1, False, 8), P(epi="qkv", controls=True, bs=16)),
    (16, 384, 1408, (1, 10, 1, False, 8), P(epi="qkv", bs=64)),
    (5, 384, 96, (1, 5, 1, False, 8), P(epi="qkv")),
    # ---- split-K slabs (each slab against its own K slice)
    (13, 272, 1408, (1, 5, 1, False, 8), P(epi="slab", ksplit=2, controls=True)),
    (32, 1360, 5248, (2, 10, 1, False, 8), P(epi="slab", ksplit=3)),
    (33, 1040, 1184, (4, 5, 2, False, 8), P(epi="slab", ksplit=4)),
    (65, 2064, 160, (6, 5, 3, False, 8), P(epi="slab", ksplit=4)),
    (33, 2064, 160, (4, 5, 3, False, 8), P(epi="slab", ksplit=4)),
    (95, 1040, 160, (6, 5, 2, False, 8), P(epi="slab", ksplit=4)),
    # ---- plain, MT 2 / 4 / 6 in one workgroup
    (17, 50, 96, (2, 5, 1, False, 8), P()),
    (31, 50, 1184, (2, 5, 1, False, 8), P(epi="gelu", controls=True)),
    (32, 4128, 1280, (2, 5, 2, False, 8), P(epi="resid", ypk=True, y_row0=16)),
    (17, 8194, 160, (2, 5, 3, False, 8), P(epi="silu")),
    (32, 50, 1408, (2, 10, 1, False, 8), P(epi="store_f32")),
    (19, 8194, 1408, (2, 10, 2, False, 8), P()),
    (17, 384, 1184, (2, 5, 1, False, 8), P(epi="qkv", bs=64)),
    (31, 64, 320, (2, 5, 1, False, 8), P(epi="relu_affine_tanh")),
    (49, 64, 320, (4, 5, 1, False, 8), P(epi="relu_affine")),
    (33, 50, 1408, (4, 10, 1, False, 8), P(epi="store_f32")),
    (81, 64, 320, (6, 5, 1, False, 8), P(epi="relu_affine_tanh")),
    (95, 384, 1184, (6, 5, 1, False, 8), P(epi="qkv", bs=32)),
    (33, 50, 96, (4, 5, 1, False, 8), P()),
    (63, 50, 1184, (4, 5, 1, False, 8), P(epi="silu")),
    (64, 64, 1280, (4, 5, 1, False, 8), P(epi="resid", copy=False)),
    (48, 50, 2720, (4, 10, 1, False, 8), P()),
    (64, 384, 1408, (4, 10, 1, False, 8), P(epi="qkv", bs=16)),
    (65, 50, 96, (6, 5, 1, False, 8), P(controls=True)),
    (95, 50, 1184, (6, 5, 1, False, 8), P(epi="gelu")),
    (96, 64, 1280, (6, 5, 1, False, 8), P(epi="resid")),
    (96, 384, 1280, (6, 5, 1, False, 8), P(epi="qkv")),
    (81, 50, 5248, (6, 10, 1, False, 8), P(epi="store_f32")),
    (97, 50, 1408, (6, 10, 1, False, 8), P()),                            # chunked: 96 rows, then 1 (MT 1)
    (130, 64, 1184, (6, 5, 1, False, 8), P(epi="resid", ypk=True)),       # chunked: 96 rows, then 34 (MT 4)
    # ---- rows dealt to grid.z
    (97, 800, 1184, (1, 5, 2, False, 8), P(rpw=16, epi="resid", ypk=True)),
    (200, 1360, 320, (1, 5, 3, False, 8), P(rpw=16, epi="gelu")),
    (256, 272, 1408, (1, 10, 2, False, 8), P(rpw=16)),
    (200, 608, 1184, (2, 5, 2, False, 8), P(rpw=32, epi="silu", ypk=True)),
    (256, 1040, 96, (2, 5, 3, False, 8), P(rpw=32)),
    (256, 528, 2720, (2, 10, 2, False, 8), P(rpw=32, epi="resid")),
    (96, 64, 1280, (2, 5, 1, False, 8), P(rpw=32, epi="resid", ypk=True)),
    # ---- LayerNorm folded into the GEMM
    (16, 64, 96, (1, 5, 1, True, 8), P(fold=True, controls=True)),
    (13, 4100, 1184, (1, 5, 2, True, 8), P(fold=True, epi="gelu")),
    (256, 528, 96, (1, 5, 3, True, 8), P(fold=True, rpw=16, ypk=False)),
    (256, 784, 1280, (1, 5, 4, True, 8), P(fold=True, rpw=16, epi="gelu")),
    (15, 64, 1408, (1, 10, 1, True, 8), P(fold=True, epi="silu")),
    (256, 272, 1312, (1, 10, 2, True, 8), P(fold=True, rpw=16)),
    (5, 384, 1280, (1, 5, 1, True, 8), P(fold=True, epi="qkv")),
    (17, 64, 1184, (2, 5, 1, True, 8), P(fold=True, ypk=True)),
    (256, 528, 1280, (2, 5, 2, True, 8), P(fold=True, rpw=32, epi="gelu", controls=True)),
    (256, 1040, 96, (2, 5, 3, True, 8), P(fold=True, rpw=32)),
    (200, 2080, 1184, (2, 5, 4, True, 8), P(fold=True, rpw=32, epi="gelu", ypk=True)),
    (32, 384, 1408, (2, 10, 1, True, 8), P(fold=True, epi="qkv", bs=16)),
    (256, 528, 1312, (2, 10, 2, True, 8), P(fold=True, rpw=32, epi="store_f32")),
    (33, 64, 96, (4, 5, 1, True, 8), P(fold=True)),
    (64, 4100, 1280, (4, 5, 2, True, 8), P(fold=True, epi="gelu")),       # NTB: 3 tiles would fit the grid rule; demoted to 2
    (63, 384, 1408, (4, 10, 1, True, 8), P(fold=True, epi="qkv")),
    (65, 64, 1184, (6, 5, 1, True, 8), P(fold=True, epi="silu")),
    (96, 8196, 320, (6, 5, 2, True, 8), P(fold=True)),                    # 513 column tiles: the grid rule asks for 3, FOLD with MT > 2 runs 2
    (95, 64, 5248, (6, 10, 1, True, 8), P(fold=True, epi="gelu")),
]
assert {(c[1], c[2], c[4].get("ksplit", 1)) for c in GEMM_CASES} == set(GEMM_SHAPES)   # the CPU planner sweep starts from these


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("case", range(len(GEMM_CASES)), ids=lambda i: "%d-M%d-N%d-K%d" % ((i,) + GEMM_CASES[i][:3]))
def test_skinny_gemm_fp64(nat, dtype, case):
    """One planned form at one edge shape against the fp64 reference (module docstring: bounds; GEMM_CASES: the shapes).

    Folded form at |mean| / sigma = 64: the bound's delta_r term is the fp32 cancellation in S2 / K - mean^2; the measured ratio of
    those rows is in profiles/decode_kernels_fp64.txt."""
    M, N, K, key, opt = GEMM_CASES[case]
    run_gemm(nat, dtype, M, N, K, key, seed=100 + 10 * case, **opt)


def test_skinny_every_plannable_form_is_pinned(nat):
    """Every instantiation plan_skinny can ask launch_skinny_mt for has a case above, in both 16-bit types (run the whole file:
    the cases fill PINNED), and no case pins a form the enumeration does not know."""
    if not PINNED:
        pytest.skip("no skinny-GEMM case ran in this process (the cases of this file fill PINNED: run the whole file)")
    for dtype in DTYPES:
        have = {k for d, k in PINNED if d == dtype}
        assert have - REACHABLE == set(), f"{tname(dtype)}: cases ran forms the enumeration calls unreachable: {sorted(have - REACHABLE)}"
        assert REACHABLE - have == set(), f"{tname(dtype)}: plannable forms no case pins: {sorted(REACHABLE - have)}"


# ------------------------------------------------------------------------------------------------- decode attention
PASS, RPW = 256, 8      # keys per pass of a 4-wave workgroup, rows per wave-load (16-bit types)


def decode_case(dtype, pads, pos, H, seed, qscale=2.0, same_q=False):
    """Logical caches [B][H][smax][64] with weight on the boundary keys (module docstring), rounded to the storage type."""
    B, smax = len(pads), pos + 9
    q = (rnd(B, H, 64, seed=seed) * qscale).to(dtype)
    if same_q:      # shared first keys: one query for every row, so that row 0's boundary keys carry weight in the rows they are copied to
        q = q[0:1].expand(B, H, 64).contiguous()
    k = rnd(B, H, smax, 64, seed=seed + 1)
    v = rnd(B, H, smax, 64, seed=seed + 2).to(dtype)
    qd = q.double()
    boost = 8.0 * 6.0 * qd / (qd * qd).sum(-1, keepdim=True)       # a key with score 6: three standard deviations up
    for b, p in enumerate(pads):
        b0 = p & ~(RPW - 1)
        marks = {p, max(p - 1, 0), pos} | set(range(b0 + PASS // 4, pos + 1, PASS // 4))
        for j in marks:
            k[b, :, j] = boost[b]
    return q, k.to(dtype), v, smax


def decode_ref(q, k, v, pads, pos, lo_shift=0, drop=None, scale=0.125):
    """fp64 softmax(q k / 8) v over the keys [pad_b + lo_shift, pos] of every row, minus the keys drop[b]; returns (ref, A)."""
    B, H, smax, _ = k.shape
    s = torch.einsum("bhd,bhjd->bhj", q.double(), k.double()) * scale
    j = torch.arange(smax, device=DEV)[None, :]
    lo = torch.tensor(pads, device=DEV)[:, None] + lo_shift
    vis = (j >= lo) & (j <= pos)
    if drop is not None:
        for b, jd in enumerate(drop):
            if jd is not None and 0 <= jd < smax:
                vis[b, jd] = False
    s = s.masked_fill(~vis[:, None, :], -math.inf)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    p = p / p.sum(-1, keepdim=True)
    ref = torch.einsum("bhj,bhjd->bhd", p, v.double())
    A = torch.einsum("bhj,bhjd->bhd", p, v.double().abs())
    return ref.reshape(B, H * 64), A.reshape(B, H * 64)


def paged_pool(k, v, pads, pos, bs, seed, swap=None):
    """The logical caches dealt into a shuffled block pool behind a 64-entry ring table; block 0 is the scratch block."""
    B, H, smax, _ = k.shape
    nb = (smax + bs - 1) // bs
    assert nb <= TAB - 2
    tab = np.zeros((B, TAB), dtype=np.int32)
    tab[:, :nb] = np.random.default_rng(seed).permutation(np.arange(1, 1 + B * nb)).reshape(B, nb)
    idx = torch.from_numpy(tab[:, :nb].astype(np.int64)).to(DEV)
    pk = torch.zeros(1 + B * nb, H, bs, 64, dtype=k.dtype, device=DEV)
    pv = torch.zeros_like(pk)
    pad_to = nb * bs - smax
    kk = torch.nn.functional.pad(k, (0, 0, 0, pad_to)).view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4)
    vv = torch.nn.functional.pad(v, (0, 0, 0, pad_to)).view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4)
    pk[idx], pv[idx] = kk, vv
    return pk, pv, tab


def unpage(pool, tab, smax, bs):
    """Logical [B][H][smax][64] view of a pool through a (possibly altered) table: what a reference with that table reads."""
    nb = (smax + bs - 1) // bs
    idx = torch.from_numpy(tab[:, :nb].astype(np.int64)).to(DEV)
    t = pool[idx].permute(0, 2, 1, 3, 4)
    return t.reshape(t.shape[0], t.shape[1], nb * bs, 64)[:, :, :smax]


# pads of one launch per context class under one *pos; slots = pos + 1 - (pad & ~7) key slots from the first group
def decode_pads(pos):
    ctx = pos + 1
    d = ctx % 8 if ctx % 8 <= 4 else ctx % 8 - 8                    # slots = ctx - b0 is congruent to ctx mod 8
    return [ctx - base - d + o for base, o in zip((PASS // 4, PASS // 2, 3 * PASS // 4, PASS), (0, 3, 5, 7))]


DECODE_LAUNCHES = [
    # (pos, pads, note)
    (303, None, "slots 64 / 128 / 192 / 256: the last slot count of arms 0-3"),
    (302, None, "slots 63 / 127 / 191 / 255"),
    (304, None, "slots 65 / 129 / 193 / 257: the first slot count of the next arm, and of a second pass"),
    (800, [0, 3, 801 - 512 - 40, 801 - 256 - 9, 800, 799, 788, 17], "three / two / one full passes plus a tail; 1, 2 and 13 keys"),
]
DECODE_FORMS = ["contiguous", "packed-out", "paged16", "paged32", "paged64", "row-table", "share", "paged16-share"]


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("form", DECODE_FORMS)
@pytest.mark.parametrize("launch", range(len(DECODE_LAUNCHES)))
def test_attn_decode_fp64(nat, dtype, form, launch):
    """Every template form of attn_decode_kernel at every arm boundary of the context-sized pass.  Rows of one launch: the four
    arm boundaries (pads no multiple of 8), a row with exactly one key (pad == *pos), a full row (pad 0), and a skipped row that
    must keep its sentinel.  Negative controls on launch 2 (a second pass exists there) for every form."""
    pos, pads, _ = DECODE_LAUNCHES[launch]
    H = 3 if form == "contiguous" else 2
    if pads is None:
        pads = decode_pads(pos) + [pos, 0, 21, 44]
    B = len(pads)
    skip_row = B - 1
    ARMS.update(decode_arm(pos + 1 - p, p) for p in pads[:-1])
    q, k, v, smax = decode_case(dtype, pads, pos, H, seed=500 + launch, same_q=form.endswith("share"))
    C, p0 = 0, 0
    share = None
    if form.endswith("share"):          # the first C keys of every row are row 0's positions [p0, p0 + C)
        C, p0 = 19, pads[0]
        for b in range(1, B):
            n = max(0, min(C, pos + 1 - pads[b], smax - p0))
            k[b, :, pads[b]:pads[b] + n] = k[0, :, p0:p0 + n]
            v[b, :, pads[b]:pads[b] + n] = v[0, :, p0:p0 + n]
        share = i32([(p0 << 8) | C])
    posd, padd = i32([pos]), i32(pads)
    skip = torch.zeros(B, dtype=torch.int32, device=DEV)
    skip[skip_row] = 1
    packed = form == "packed-out"
    out = torch.full(((B + 15) // 16 * 16 * H * 64,) if packed else (B, H * 64), 7.0, dtype=dtype, device=DEV)
    qf = q.reshape(B, H * 64).contiguous()
    tab = bs = None
    if form.startswith("paged"):
        bs = int(form[5:7])
        pk, pv, tab = paged_pool(k, v, pads, pos, bs, seed=launch)
        if C:       # the rows' own copies of the shared keys hold garbage: they must be read from row 0's blocks
            junk_k, junk_v = k.clone(), v.clone()
            for b in range(1, B):
                n = max(0, min(C, pos + 1 - pads[b]))
                junk_k[b, :, pads[b]:pads[b] + n] = 3.0
                junk_v[b, :, pads[b]:pads[b] + n] = 3.0
            pk, pv, tab = paged_pool(junk_k, junk_v, pads, pos, bs, seed=launch)
        nat.attn_decode(qf, pk, pv, out, padd, posd, B, H, 0, skip_rows=skip, kv_share=share, kv_tab=i32(tab), kv_bs=bs)
    elif form == "row-table":           # position j of logical row b lives in physical row table[parity][b][j]
        g = torch.Generator().manual_seed(launch)
        t1 = torch.stack([torch.randperm(B, generator=g) for _ in range(smax)], 1).to(DEV)      # [B][smax], a permutation per position
        kp, vp = torch.zeros_like(k), torch.zeros_like(v)
        jj = torch.arange(smax, device=DEV)[None, :].expand(B, smax)
        kp[t1, :, jj], vp[t1, :, jj] = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        t0 = torch.roll(t1, 1, 0)                                                                 # the other parity: another row's table
        tbl = torch.stack([t0, t1]).to(torch.int32).contiguous()
        nat.attn_decode(qf, kp, vp, out, padd, posd, B, H, smax, skip_rows=skip, kv_rows=tbl, kv_step=i32([1]))
    else:
        kc, vc = k, v
        if C:
            kc, vc = k.clone(), v.clone()
            for b in range(1, B):
                n = max(0, min(C, pos + 1 - pads[b]))
                kc[b, :, pads[b]:pads[b] + n] = 3.0
                vc[b, :, pads[b]:pads[b] + n] = 3.0
        nat.attn_decode(qf, kc, vc, out, padd, posd, B, H, smax, out_packed=packed, skip_rows=skip, kv_share=share)
    got = nat.unpack_activation(out, B, H * 64) if packed else out
    what = f"attn_decode {tname(dtype)} {form} pos={pos} pads={pads}"
    assert (got[skip_row] == 7.0).all(), f"{what}: the skipped row was written"
    valid = torch.ones(B, 1, dtype=torch.bool, device=DEV)
    valid[skip_row] = False
    ref, A = decode_ref(q, k, v, pads, pos)
    bound = ulp(ref, dtype) + C_ATTN * A
    ok(what, got, ref, bound, valid)
    if launch != 2:
        return

    def dbad(control, r):      # a control that leaves a row without any key says nothing about that row
        fin = torch.isfinite(r).all(1, keepdim=True)
        bad(what, control, got, torch.nan_to_num(r), bound, valid & fin)
    b0s = [p & ~(RPW - 1) for p in pads]
    dbad("the key at pad[b] left out", decode_ref(q, k, v, pads, pos, lo_shift=1)[0])
    dbad("the key at pad[b] - 1 let in", decode_ref(q, k, v, pads, pos, lo_shift=-1)[0])
    dbad("the key at *pos left out", decode_ref(q, k, v, pads, pos, drop=[pos if p < pos else None for p in pads])[0])
    dbad("the first key of the second pass left out", decode_ref(q, k, v, pads, pos, drop=[b0 + PASS if b0 + PASS <= pos else None for b0 in b0s])[0])
    dbad("scale 1/8 (1 + 2^-9)", decode_ref(q, k, v, pads, pos, scale=0.125 * (1 + 2.0 ** -9))[0])
    if C:
        k2, v2 = k.clone(), v.clone()
        for b in range(1, B):
            n = max(0, min(C, pos + 1 - pads[b]))
            k2[b, :, pads[b]:pads[b] + n] = k[0, :, p0 + 1:p0 + 1 + n]
            v2[b, :, pads[b]:pads[b] + n] = v[0, :, p0 + 1:p0 + 1 + n]
        dbad("the shared keys taken from p0 + 1", decode_ref(q, k2, v2, pads, pos)[0])
    if form == "row-table":
        idx = t0[:, None, :, None].expand(B, H, smax, 64)
        dbad("the table of the other parity", decode_ref(q, torch.gather(kp, 0, idx), torch.gather(vp, 0, idx), pads, pos)[0])
    if tab is not None and not C:
        t2 = tab.copy()
        e = pos // bs          # the block of *pos and its neighbour: inside the window attention does not see a permutation of (k, v) pairs
        t2[:, [e, e - 1]] = tab[:, [e - 1, e]]
        dbad("one block entry exchanged with its neighbour", decode_ref(q, unpage(pk, t2, smax, bs), unpage(pv, t2, smax, bs), pads, pos)[0])


# ------------------------------------------------------------------------------------------------- prefill attention
def prefill_ref(q, k, v, qpos, lo, drop=None, causal_shift=0):
    """fp64 attention of queries q [Q][H][64] at sequence positions qpos [Q] over keys k / v [J][H][64] (storage type): key j visible
    iff lo <= j <= qpos + causal_shift (and j not in drop).  Walks the kernel's 64-key tiles from sequence position 0 with the
    running maximum and rounds P = exp(s - m) to the storage type where the kernel does (the row sum takes the unrounded P).
    Returns (ref [Q][H*64], A, E, visible count) with E the fp32-level budget of `prefill_bound` (module docstring): the midpoint
    allowance plus the score / exp / sum term.  Rows without a key: zeros."""
    dtype = v.dtype
    Q, H, _ = q.shape
    J = k.shape[0]
    s = torch.einsum("qhd,jhd->hqj", q.double(), k.double()) * 0.125
    T = torch.einsum("qhd,jhd->hqj", q.double().abs(), k.double().abs()) * 0.125      # sum_d |q_d k_jd| / 8: what a score's error scales with
    j = torch.arange(J, device=DEV)[None, :]
    vis = (j >= lo) & (j <= (qpos[:, None] + causal_shift))
    if drop is not None:
        vis[:, drop] = False
    s = s.masked_fill(~vis[None], -math.inf)
    T = T * vis[None]
    Tmax = T.max(-1, keepdim=True).values
    delta = 2.0 ** -21 * (T + Tmax) + 2.0 ** -19                   # relative distance of the kernel's fp32 P_j from the float64 P_j
    vd = v.double().transpose(0, 1)                               # [H][J][64]
    state = walk_start(H, Q, DEV)
    for jt in range(0, J, 64):
        state, _ = walk_step(state, s[:, :, jt:jt + 64], delta[:, :, jt:jt + 64], vd[:, jt:jt + 64], dtype, sum_rounded=False)
    _, l, O, Ab, Em, Ed, dbar, _ = state
    inv = torch.where(l > 0, 1.0 / torch.clamp(l, min=1e-300), torch.zeros_like(l))
    out = lambda t: (t * inv).transpose(0, 1).reshape(Q, H * 64)  # noqa: E731
    ref, A = out(O), out(Ab)
    E = out(Em) + out(Ed) + out(dbar.expand(H, Q, 64)) * ref.abs()
    return ref, A, E, vis.sum(-1)


def prefill_bound(ref, A, E, dtype):
    return ulp(ref, dtype) + E


def split_qkv(qkv, H):
    D = H * 64
    return tuple(t.reshape(-1, H, 64) for t in qkv.split(D, dim=-1))


def prefill_inputs(rows, H, dtype, seed, qscale=2.0):
    """qkv [rows][3 H 64]; q scaled so that scores have a standard deviation of 2 (f16: spread well past 14 ln 2, subnormal P)."""
    D = H * 64
    t = rnd(rows, 3 * D, seed=seed)
    t[:, :D] *= qscale
    return t.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_attn_prefill_left_padded_fp64(nat, dtype, S):
    """itts_attn_prefill: pads 0, 5, 63, 64, 70 in one launch (a tile wholly inside the padding, a tile straddling it, rows with
    no visible key: exact zeros).  Cache: positions [64 floor(pad / 64), S) hold the k / v thirds bit for bit (the kernel walks key
    tiles from the padding's tile), every other position keeps its sentinel.  At f16 the scores spread over ~24 > 14 ln 2."""
    H, smax = 2, 136
    pads = [0, 5, 63, 64, 70]
    B, D = len(pads), 128
    qkv = prefill_inputs(B * S, H, dtype, seed=700 + S, qscale=4.0 if dtype == F16 else 2.0).view(B, S, 3 * D)
    out = torch.full((B, S, D), 7.0, dtype=dtype, device=DEV)
    kc = torch.full((B, H, smax, 64), 7.0, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, 7.0)
    nat.attn_prefill(qkv, out, kc, vc, i32(pads), B, S, H, smax)
    qpos = torch.arange(S, device=DEV)
    for b, pad in enumerate(pads):
        q, k, v = split_qkv(qkv[b], H)
        what = f"attn_prefill {tname(dtype)} S={S} pad={pad}"
        ref, A, allow, nvis = prefill_ref(q, k, v, qpos, pad)
        bound = prefill_bound(ref, A, allow, dtype)
        ok(what, out[b], ref, bound)
        assert (out[b][nvis == 0] == 0).all(), f"{what}: a row without a visible key is not exact zeros"
        first = min((pad // 64) * 64, S)
        for cache, src in ((kc, k), (vc, v)):
            assert torch.equal(cache[b, :, first:S], src[first:S].transpose(0, 1)), f"{what}: cache rows differ from the k / v thirds"
            assert (cache[b, :, :first] == 7.0).all() and (cache[b, :, S:] == 7.0).all(), f"{what}: a cache position outside the rows was written"
        if S == 130 and pad in (5, 70):
            valid = (nvis > 0)[:, None]
            bad(what, "key i + 1 visible to query i", out[b], prefill_ref(q, k, v, qpos, pad, causal_shift=1)[0], bound, valid)
            bad(what, "the key at pad - 1 let in", out[b], prefill_ref(q, k, v, qpos, pad - 1)[0], bound, valid)
            if pad == 5:
                bad(what, "the key at position 64 left out", out[b], prefill_ref(q, k, v, qpos, pad, drop=[64])[0], bound, valid)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("paged", [0, 16])
def test_attn_prefill_packed_fp64(nat, dtype, paged):
    """itts_attn_prefill_packed: elements of 1, 64 and 65 rows in one launch, cache row of local row i = cache_shift[b] + i."""
    H, smax = 2, 96
    lens, shift = [1, 64, 65], [7, 0, 19]
    B, D = len(lens), 128
    off = np.concatenate([[0], np.cumsum(lens)])
    qkv = prefill_inputs(int(off[-1]), H, dtype, seed=720)
    out = torch.full((int(off[-1]), D), 7.0, dtype=dtype, device=DEV)
    if paged:
        nb = smax // paged
        tab = np.zeros((B, TAB), dtype=np.int32)
        tab[:, :nb] = np.random.default_rng(1).permutation(np.arange(1, 1 + B * nb)).reshape(B, nb)
        kc = torch.full((1 + B * nb, H, paged, 64), 7.0, dtype=dtype, device=DEV)
        vc = torch.full_like(kc, 7.0)
        nat.attn_prefill_packed(qkv, out, kc, vc, i32(off), i32(shift), B, max(lens), H, 0, kv_tab=i32(tab), kv_bs=paged)
        kl, vl = unpage(kc, tab, smax, paged), unpage(vc, tab, smax, paged)
        assert (kc[0] == 7.0).all() and (vc[0] == 7.0).all()
    else:
        kc = torch.full((B, H, smax, 64), 7.0, dtype=dtype, device=DEV)
        vc = torch.full_like(kc, 7.0)
        nat.attn_prefill_packed(qkv, out, kc, vc, i32(off), i32(shift), B, max(lens), H, smax)
        kl, vl = kc, vc
    for b, n in enumerate(lens):
        rows = slice(int(off[b]), int(off[b + 1]))
        q, k, v = split_qkv(qkv[rows], H)
        what = f"attn_prefill_packed {tname(dtype)} paged={paged} len={n}"
        ref, A, allow, _ = prefill_ref(q, k, v, torch.arange(n, device=DEV), 0)
        bound = prefill_bound(ref, A, allow, dtype)
        ok(what, out[rows], ref, bound)
        for cache, src in ((kl, k), (vl, v)):
            assert torch.equal(cache[b, :, shift[b]:shift[b] + n], src.transpose(0, 1)), f"{what}: cache rows differ from the k / v thirds"
            assert (cache[b, :, :shift[b]] == 7.0).all() and (cache[b, :, shift[b] + n:] == 7.0).all(), f"{what}: stray cache write"
        if n == 65:
            bad(what, "key i + 1 visible to query i", out[rows], prefill_ref(q, k, v, torch.arange(n, device=DEV), 0, causal_shift=1)[0], bound)
            bad(what, "the key at position 64 left out", out[rows], prefill_ref(q, k, v, torch.arange(n, device=DEV), 0, drop=[64])[0], bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("paged", [0, 32])
def test_attn_prefill_prefix_fp64(nat, dtype, paged):
    """itts_attn_prefill_prefix: prefix lengths 0, 1, 63, 64, 100 read from cache rows (permuted, at an offset), contiguous and paged;
    the caches are read only."""
    H, smax = 2, 128
    pre, mq = [0, 1, 63, 64, 100], [5, 64, 65, 1, 70]
    crow, pos0 = [3, 0, 4, 1, 2], [9, 0, 11, 3, 20]
    B, D = len(pre), 128
    off = np.concatenate([[0], np.cumsum(mq)])
    qkv = prefill_inputs(int(off[-1]), H, dtype, seed=740)
    ck = rnd(B, H, smax, 64, seed=741).to(dtype)
    cv = rnd(B, H, smax, 64, seed=742).to(dtype)
    out = torch.full((int(off[-1]), D), 7.0, dtype=dtype, device=DEV)
    if paged:
        pk, pv, tab = paged_pool(ck, cv, None, None, paged, seed=2)
        pk0, pv0 = pk.clone(), pv.clone()
        nat.attn_prefill_prefix(qkv, out, pk, pv, i32(off), i32(pre), i32(crow), i32(pos0), B, max(mq), H, 0, kv_tab=i32(tab), kv_bs=paged)
        assert torch.equal(pk, pk0) and torch.equal(pv, pv0)
    else:
        ck0, cv0 = ck.clone(), cv.clone()
        nat.attn_prefill_prefix(qkv, out, ck, cv, i32(off), i32(pre), i32(crow), i32(pos0), B, max(mq), H, smax)
        assert torch.equal(ck, ck0) and torch.equal(cv, cv0)
    for b in range(B):
        rows = slice(int(off[b]), int(off[b + 1]))
        q, k, v = split_qkv(qkv[rows], H)
        what = f"attn_prefill_prefix {tname(dtype)} paged={paged} pre={pre[b]} rows={mq[b]}"

        def seq(p_from, n=pre[b], b=b, k=k, v=v):
            kp = ck[crow[b], :, p_from:p_from + n].transpose(0, 1)
            vp = cv[crow[b], :, p_from:p_from + n].transpose(0, 1)
            return torch.cat([kp, k]), torch.cat([vp, v])
        kk, vv = seq(pos0[b])
        qpos = pre[b] + torch.arange(mq[b], device=DEV)
        ref, A, allow, _ = prefill_ref(q, kk, vv, qpos, 0)
        bound = prefill_bound(ref, A, allow, dtype)
        ok(what, out[rows], ref, bound)
        if pre[b] in (1, 100):
            bad(what, "prefix key pre_len - 1 left out", out[rows], prefill_ref(q, kk, vv, qpos, 0, drop=[pre[b] - 1])[0], bound)
            k1, v1 = seq(pos0[b] + 1)
            bad(what, "the prefix read from pre_pos0 + 1", out[rows], prefill_ref(q, k1, v1, qpos, 0)[0], bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
def test_attn_prefill_shared_fp64(nat, dtype):
    """itts_attn_prefill_shared: element 0 is the shared block (prefix length 0), elements 1-3 sit behind prefixes that are rows of qkv
    itself (lengths 63, 64 and 30 -- element 3 behind a different slice of the block); own rows appended to the caches."""
    H, smax = 2, 160
    lens = [70, 1, 65, 64]
    pre, pre_row0 = [0, 63, 64, 30], [0, 0, 0, 5]
    w_row, w_pos0 = [0, 1, 2, 3], [3, 70, 64, 40]
    E, D = len(lens), 128
    off = np.concatenate([[0], np.cumsum(lens)])
    qkv = prefill_inputs(int(off[-1]), H, dtype, seed=760)
    out = torch.full((int(off[-1]), D), 7.0, dtype=dtype, device=DEV)
    kc = torch.full((E, H, smax, 64), 7.0, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, 7.0)
    nat.attn_prefill_shared(qkv, out, kc, vc, i32(off), i32(pre), i32(pre_row0), i32(w_row), i32(w_pos0), E, max(lens), H, smax)
    qa, ka, va = split_qkv(qkv, H)
    for e in range(E):
        rows = slice(int(off[e]), int(off[e + 1]))
        what = f"attn_prefill_shared {tname(dtype)} element {e} pre={pre[e]} rows={lens[e]}"

        def seq(r0, e=e, rows=rows):
            return torch.cat([ka[r0:r0 + pre[e]], ka[rows]]), torch.cat([va[r0:r0 + pre[e]], va[rows]])
        kk, vv = seq(pre_row0[e])
        qpos = pre[e] + torch.arange(lens[e], device=DEV)
        ref, A, allow, _ = prefill_ref(qa[rows], kk, vv, qpos, 0)
        bound = prefill_bound(ref, A, allow, dtype)
        ok(what, out[rows], ref, bound)
        for cache, src in ((kc, ka), (vc, va)):
            assert torch.equal(cache[w_row[e], :, w_pos0[e]:w_pos0[e] + lens[e]], src[rows].transpose(0, 1)), f"{what}: appended rows differ"
            assert (cache[w_row[e], :, :w_pos0[e]] == 7.0).all() and (cache[w_row[e], :, w_pos0[e] + lens[e]:] == 7.0).all(), f"{what}: stray write"
        if e == 2:
            k3, v3 = seq(pre_row0[3])
            bad(what, "pre_row0 of element 3 given to element 2", out[rows], prefill_ref(qa[rows], k3, v3, qpos, 0)[0], bound)
            bad(what, "prefix key pre_len - 1 left out", out[rows], prefill_ref(qa[rows], kk, vv, qpos, 0, drop=[pre[e] - 1])[0], bound)


# ------------------------------------------------------------------------------------------------- row kernels
C_LN = 2.0 ** -20


def ln_ref(x, w, b, eps=1e-5, cols=None, e_in=None):
    """fp64 LayerNorm of the rows x [M][D] (statistics over the first `cols` columns: all by default) and its fp32-level budget.

    Derivation, from the two-pass statistics of ln_math.h / ln_reduce_kernel / layernorm_kernel (u = 2^-24).  mean: per-lane sums,
    six shuffle levels and the cross-wave sum, an fp32 chain: |dmean| <= 2^-21 E|x| (the chain figure of the GEMM bound).  The
    squares are taken of d = x - mean, CENTRED, so q = sum d^2 has no cancellation: a common error of the d enters q only in second
    order (sum d = 0), the chain adds 2^-21 relative, rsqrtf one ulp: rstd is 2^-22 + 2^-23 relative.  d itself carries u, and
    y = d rstd w + b three more roundings on |y - b| and one, the last addition, on |y|.  Together
        |y - ref| <= C_LN |ref - b| + 2^-21 |w| rstd E|x| + 2^-24 |ref|,     C_LN = 2^-20  (u + 2^-22 + 2^-23 + 3 u = 0.63 x 2^-20).
    e_in (second LayerNorm of a pair): per-element error bound of x itself; a perturbation e moves the output by
    rstd w (e_i - mean e - n_i mean(n e)), n the normalised row: <= |w| rstd (e_i + mean e + |n_i| rms e)."""
    xd, wd, bd = x.double(), w.double(), b.double()
    xs = xd if cols is None else xd[:, :cols]
    mean = xs.mean(1, keepdim=True)
    var = ((xs - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    n = (xd - mean) * rstd
    ref = n * wd + bd
    E = C_LN * (ref - bd).abs() + 2.0 ** -21 * wd.abs() * rstd * xd.abs().mean(1, keepdim=True) + 2.0 ** -24 * ref.abs()
    if e_in is not None:
        E = E + wd.abs() * rstd * (e_in + e_in.mean(1, keepdim=True) + n.abs() * torch.sqrt((e_in ** 2).mean(1, keepdim=True)))
    return ref, E


def fma32(t, b, v):
    """fmaf(t, b, v) of fp32 tensors: the product of two fp32 values is exact in float64."""
    return (t.double() * b.double() + v.double()).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("ypk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("M", [1, 13, 32, 96])
def test_ln_reduce_fp64(nat, dtype, M, ypk):
    """itts_ln_reduce: nslab 0 / 3 / 6, bias, the second LayerNorm, lora_b with r = 4 / 16 / 24 (by M) behind slabs that are
    slab_stride = D + 16 ceil(r / 16) > D wide, D = 1280 (five waves per row) and D = 320 (the one-wave form, row-major only).
    h after the slab sum is the fixed-order fp32 sum bit for bit; the output is held to ln_ref's bound.  Row 0 has a small variance
    (sigma 0.01: eps matters there).  Controls on M = 13."""
    r = {1: 4, 13: 16, 32: 24, 96: 16}[M]
    configs = [(1280, 0, False, 0, False), (1280, 3, True, r, False), (1280, 6, True, 0, True), (1280, 3, False, 0, True), (256, 6, True, r, True)]
    if not ypk:
        configs.append((320, 3, True, 0, True))
    for ci, (D, nslab, has_bias, lr, two) in enumerate(configs):
        seed = 3000 + 20 * ci + M
        stride = D + 16 * ((lr + 15) // 16) if lr else (D + 64 if (nslab == 6 and D == 1280) else D)
        h0 = (rnd(M, D, seed=seed, scale=2.0) + 0.3).float()
        h0[0] = (rnd(D, seed=seed + 1) * 0.01 + 0.5).float()
        slab = rnd(max(nslab, 1), M, stride, seed=seed + 2, scale=0.5 if M > 1 or nslab == 0 else 0.001).float()
        if nslab:
            slab[:, 0] *= 0.002        # row 0 keeps its small variance through the update
        bias = (rnd(D, seed=seed + 3) * 0.001).float() if has_bias else None
        lw, lb = (1 + 0.1 * rnd(D, seed=seed + 4)).float(), (0.1 * rnd(D, seed=seed + 5)).float()
        lw2, lb2 = ((1 + 0.1 * rnd(D, seed=seed + 6)).float(), (0.1 * rnd(D, seed=seed + 7)).float()) if two else (None, None)
        lora_b = (rnd(lr, D, seed=seed + 8) * 0.05).float() if lr else None
        h = h0.clone()
        out = torch.full((nat.packed_rows(M) * D,) if ypk else (M, D), 7.0, dtype=dtype, device=DEV)
        nat.ln_reduce(h, lw, lb, out, slab=slab if nslab else None, nslab=nslab, bias=bias, w2=lw2, b2=lb2, y_packed=ypk,
                      slab_stride=stride if stride != D else 0, lora_b=lora_b)
        got = nat.unpack_activation(out, M, D) if ypk else out
        what = f"ln_reduce {tname(dtype)} M={M} D={D} nslab={nslab} bias={has_bias} r={lr} ln2={two} stride={stride} packed={ypk}"

        def h_of(slabs, lb_=lora_b):
            v = h0.clone()
            if not slabs:
                return v
            if bias is not None:
                v = v + bias
            for i in slabs:
                v = v + slab[i][:, :D]
            if lb_ is not None:
                for j in range(lr):
                    t = torch.zeros(M, device=DEV)
                    for i in slabs:
                        t = t + slab[i][:, D + j]
                    v = fma32(t[:, None], lb_[j][None, :], v)
            return v
        h_ref = h_of(list(range(nslab)))
        assert torch.equal(h, h_ref), f"{what}: h is not the fixed-order fp32 sum"

        def y_of(hh, eps=1e-5, cols=None):
            ref, E = ln_ref(hh, lw, lb, eps, cols)
            if two:
                ref, E = ln_ref(ref, lw2, lb2, eps, cols, e_in=E)
            return ref, ulp(ref, dtype) + E
        ref, bound = y_of(h_ref)
        ok(what, got, ref, bound)
        if M != 13:
            continue
        bad(what, "statistics over D - 4 columns", got, y_of(h_ref, cols=D - 4)[0], bound)
        bad(what, "eps of 1e-6", got, y_of(h_ref, eps=1e-6)[0], bound)
        if nslab:
            bad(what, "one slab missing", got, y_of(h_of(list(range(nslab - 1))))[0], bound)
        if lr:
            sw = lora_b.clone()
            sw[[lr - 2, lr - 1]] = lora_b[[lr - 1, lr - 2]]
            bad(what, "the last two rows of lora_b exchanged", got, y_of(h_of(list(range(nslab)), sw))[0], bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("M", [1, 13, 32, 96])
def test_layernorm_fp64(nat, dtype, M):
    """itts_layernorm with and without the second pair, D = 1280 and D = 320."""
    for D in (1280, 320):
        for two in (False, True):
            seed = 3500 + M + D
            h = (rnd(M, D, seed=seed, scale=2.0) + 0.3).float()
            h[0] = (rnd(D, seed=seed + 1) * 0.01 + 0.5).float()
            lw, lb = (1 + 0.1 * rnd(D, seed=seed + 4)).float(), (0.1 * rnd(D, seed=seed + 5)).float()
            lw2, lb2 = ((1 + 0.1 * rnd(D, seed=seed + 6)).float(), (0.1 * rnd(D, seed=seed + 7)).float()) if two else (None, None)
            out = torch.full((M, D), 7.0, dtype=dtype, device=DEV)
            nat.layernorm(h, lw, lb, out, w2=lw2, b2=lb2)

            def y_of(eps=1e-5, cols=None):
                ref, E = ln_ref(h, lw, lb, eps, cols)
                if two:
                    ref, E = ln_ref(ref, lw2, lb2, eps, cols, e_in=E)
                return ref, ulp(ref, dtype) + E
            ref, bound = y_of()
            what = f"layernorm {tname(dtype)} M={M} D={D} ln2={two}"
            ok(what, out, ref, bound)
            if M == 13:
                bad(what, "statistics over D - 4 columns", out, y_of(cols=D - 4)[0], bound)
                bad(what, "eps of 1e-6", out, y_of(eps=1e-6)[0], bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("B", [1, 13, 32, 96])
def test_embed_step_exact(nat, dtype, B):
    """itts_embed_step: h = table[token] + pos_table[p] is one fp32 addition (bit-exact), the packed copy is that row rounded to the
    storage type bit for bit, p = clamp(*step - row_step0[b] + pos_add, 0, rows - 1) is clamped at both ends, the word is bumped once."""
    D, V, PR, step, pos_add = 1280, 50, 20, 7, 1
    table, ptab = rnd(V, D, seed=3700).float(), rnd(PR, D, seed=3701).float()
    g = torch.Generator().manual_seed(B)
    tok = torch.randint(0, V, (B,), generator=g).to(torch.int32).to(DEV)
    s0 = [(0, 100, -10000, 3, 8, 7, -12, 9)[i % 8] for i in range(B)]          # p = 8, < 0, >= rows, 5, 0, 1, 20 -> 19, -1 -> 0
    mtp = (B + 15) // 16
    h = torch.full((B, D), 7.0, device=DEV)
    hp = torch.full((mtp * 16 * D,), 7.0, dtype=dtype, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    nat.embed_step(tok, table, ptab, i32([step]), pos_add, h, bump=word, row_step0=i32(s0), h_packed=hp)
    p = torch.tensor([min(max(step - v + pos_add, 0), PR - 1) for v in s0], device=DEV)
    ref = table[tok.long()] + ptab[p]
    assert torch.equal(h, ref), "h is not table[token] + pos_table[p]"
    assert torch.equal(nat.unpack_activation(hp, B, D), ref.to(dtype)), "the packed copy is not the rounded fp32 row"
    assert word.item() == 1
    if B == 13:
        wrong = table[tok.long()] + ptab[torch.clamp(p + 1, max=PR - 1)]
        assert not torch.equal(h, wrong)


# ------------------------------------------------------------------------------------------------- production coverage
ARMS = set()            # arms of the context-sized pass the decode cases above ran (filled from their pads)


def decode_arm(ctx_keys, pad):
    """Arm of attn_decode_kernel's context-sized first pass for a row with `ctx_keys` keys from pad: slots from pad & ~7."""
    slots = ctx_keys + (pad & (RPW - 1))
    return min((slots - 1) // (PASS // 4), 3)


@pytest.fixture(scope="module")
def production(nat):
    """Arguments of every nat.gemm_skinny call of one _step_transformer of a 2-layer full-width bf16 engine (D = 1280, H = 20,
    V = 8194; synthetic weights) in five configurations: B = 1, B = 32 fold, B = 32 launch, B = 96, B = 32 with a LoRA bank of 8
    adapters of rank 16."""
    import os

    import synth
    import test_lora_bank_gpu as lb
    import weights
    sd = weights.gpt_state_dict(2)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt_small.npz"))
    text1 = torch.from_numpy(g["text"][0:1, :int(g["text_lens"][0])]).to(DEV)
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    rec = {}
    g0 = nat.gemm_skinny

    def record(name, m, B, **kw):
        eng = m.engine
        conds = m.get_conditioning(cond_mel, None)
        emb, pad = m.prefix_rows(conds, text1.repeat(B, 1))
        eng.prefill(emb, pad, 8, **kw)
        calls = []

        def wrapped(dtype, M, N, K, wp, bias=None, **k):
            calls.append(dict(dtype=dtype, M=M, N=N, K=K, epi=k.get("epi", 0), ksplit=k.get("ksplit", 1), rpw=k.get("rows_per_wg", 0),
                              wide=bool(k.get("wide_wg", False)), fold=k.get("ln_c") is not None, xpk=bool(k.get("x_packed", False)),
                              ypk=bool(k.get("y_packed", False)), bs=int(k.get("kv_bs", 0)) if k.get("kv_tab") is not None else 0,
                              copy=k.get("y") is not None))
            g0(dtype, M, N, K, wp, bias, **k)
        nat.gemm_skinny = wrapped
        try:
            eng._step_transformer(B, gemm_only=True)
            torch.cuda.synchronize()
        finally:
            nat.gemm_skinny = g0
        rec[name] = (eng.decode_mode, calls)

    m = lb.make_model(sd, BF16)
    record("B=1", m, 1)
    record("B=32 fold", m, 32)
    record("B=96", m, 96)
    old = os.environ.get("ITTS_DECODE_MODE")
    os.environ["ITTS_DECODE_MODE"] = "launch"
    try:
        ml = lb.make_model(sd, BF16)
    finally:
        if old is None:
            del os.environ["ITTS_DECODE_MODE"]
        else:
            os.environ["ITTS_DECODE_MODE"] = old
    record("B=32 launch", ml, 32)
    del ml
    bank, _ = lb.make_bank(sd, (16,) * 8, (1.0,) * 8)
    m.attach_lora_bank(bank)
    record("B=32 bank", m, 32, adapter_ids=[i % 9 - 1 for i in range(32)])
    del m
    return rec


def test_production_skinny_forms_are_pinned_and_hold_fp64(nat, production):
    """Every skinny-GEMM call of a production decode step maps to a form key the edge matrix pins (run the whole file: the cases
    fill PINNED), and every distinct signature (shape, epilogue, launch hints, layouts) passes the fp64 check of run_gemm."""
    if not PINNED:
        pytest.skip("no skinny-GEMM case ran in this process (the cases of this file fill PINNED: run the whole file)")
    assert production["B=32 fold"][0] == "fold" and production["B=32 launch"][0] == "launch"
    names = {nat.EPI_QKV_CACHE: "qkv", nat.EPI_GELU_STORE: "gelu", nat.EPI_RESID_F32: "resid", nat.EPI_SLAB_F32: "slab",
             nat.EPI_STORE_F32: "store_f32"}
    seen, missing = {}, []
    for cfg, (_, calls) in production.items():
        assert len(calls) == 2 * 4 + 1, (cfg, len(calls))
        for c in calls:
            assert c["dtype"] == BF16, (cfg, c)
            key = form_key(nat, BF16, c["M"], c["N"], c["K"], c["ksplit"], c["rpw"], c["wide"], c["fold"])
            print(f"production | {cfg} | M={c['M']} N={c['N']} K={c['K']} {names[c['epi']]} ksplit={c['ksplit']} rows_per_wg={c['rpw']} "
                  f"wide={c['wide']} fold={c['fold']} -> {key}")
            if (BF16, key) not in PINNED:
                missing.append((cfg, c, key))
            sig = tuple(sorted((k, str(v)) for k, v in c.items()))
            seen.setdefault(sig, (c, key))
    assert not missing, f"production calls whose form no edge case pins: {missing}"
    assert any(c["fold"] for c, _ in seen.values()) and any(c["ksplit"] > 1 for c, _ in seen.values()) and any(c["K"] == 1408 for c, _ in seen.values())
    for i, (c, key) in enumerate(seen.values()):
        run_gemm(nat, BF16, c["M"], c["N"], c["K"], key, epi=names[c["epi"]], ksplit=c["ksplit"], rpw=c["rpw"], wide=c["wide"], fold=c["fold"],
                 ypk=c["ypk"], copy=c["copy"], bs=c["bs"], seed=9000 + 10 * i, pin=False)


def test_production_attention_arms_are_pinned_and_hold_fp64(nat):
    """The contexts attention.hip quotes for the decode loop -- 1, 75 and 216 keys -- select arms the decode cases above ran, and
    hold the fp64 bound at the production head count (H = 20), packed output as the engine asks for it."""
    if not ARMS:
        pytest.skip("no decode-attention case ran in this process (run the whole file)")
    pos, ctxs = 300, (1, 75, 216)
    pads = [pos + 1 - c for c in ctxs]
    arms = [decode_arm(c, p) for c, p in zip(ctxs, pads)]
    print("production | attention arms of contexts", ctxs, "->", arms)
    assert set(arms) <= ARMS, (arms, sorted(ARMS))
    assert arms[0] == 0 and arms[2] == 3
    for dtype in DTYPES:
        q, k, v, smax = decode_case(dtype, pads, pos, 20, seed=9500)
        out = torch.full((16 * 20 * 64,), 7.0, dtype=dtype, device=DEV)
        nat.attn_decode(q.reshape(3, 1280).contiguous(), k, v, out, i32(pads), i32([pos]), 3, 20, smax, out_packed=True)
        ref, A = decode_ref(q, k, v, pads, pos)
        ok(f"attn_decode {tname(dtype)} production contexts {ctxs} H=20", nat.unpack_activation(out, 3, 1280), ref, ulp(ref, dtype) + C_ATTN * A)
