"""fp64 parity of the FP8 (E4M3 weight-only) skinny-GEMM forms, itts_gemm_skinny_w8 (include/indextts_hip.h), element by
element, with the bound model of test_decode_kernels_gpu.py.

The operands are exact: x is rounded to the activation type, the weights are E4M3 codes (every finite one is a bf16 and an f16
value), so the MFMAs accumulate exact products in fp32 as in the 16-bit kernel and the same accumulation bound holds for the
unscaled sum.  The kernel multiplies that sum by w_scale[n] in front of the epilogue, which multiplies the bound by |w_scale[n]|:
the reference is the float64 GEMM over the dequantised weights w_scale . decode(codes), whose |x| |w| sums carry the factor.
      T output:      |y - ref| <= ulp_T(ref) + 2^-21 S        S = sum_k |x| |w_scale decode| + |bias| (+ |resid|)
      fp32 output:   |y - ref| <= 2^-21 S
      gelu:          |y - ref| <= ulp_T(ref) + 1.13 2^-21 S + 2^-21 |ref|
      folded:        v = rstd (w_scale acc - mean ln_c) + d with ln_c = w_scale . sum_k decode (float64 sums), the bound of the 16-bit
                     folded form (gemm_pre) over the dequantised weights.
Shapes.  M in {1, 16, 33, 96} (33: a ragged row tile, 96: all six), K in {64, 96, 1280} (96: the image's K padding, 1280: several
blocks per wave), N in {16, 20, 50} (20: a partial column tile; 50: N % 4 != 0, STORE_F32 only).  Two epilogues cannot run at those
N and get the smallest N they accept: a packed y needs N % 32 == 0 (N = 64) and the QKV epilogue N = 3 . heads . 64 (N = 192).
The forms those shapes do not reach (2-4 column tiles per workgroup, 5 blocks per pass) are reached at wider N and K = 1664 by
test_every_built_form, which holds the cases it finds against the list of instantiations (REACHABLE_W8).
Every check prints one line `fp64 | kind | case | worst err / bound`; profiles/w8_kernels_fp64.txt is that output."""
import math

import numpy as np
import pytest
import torch

from fp64_check import bad, fold_rows, ok, rnd, tname, ulp
from test_decode_kernels_gpu import gelu_new, gemm_pre

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [BF16, F16]
TAB = 64

# Every instantiation launch_skinny_w8_mt can be asked for (MT, blocks per pass, column tiles, FOLD), by plan_skinny_w8's rules:
#   3 blocks: 1, 2, 3 tiles -- 3 not with FOLD and MT > 2 --, 4 only with FOLD and MT <= 2;   5 blocks: 1 tile, 2 only with MT <= 2.
REACHABLE_W8 = set()
for _mt in (1, 2, 4, 6):
    for _fold in (False, True):
        for _ntb in (1, 2, 3, 4):
            if (_ntb == 3 and _fold and _mt > 2) or (_ntb == 4 and not (_fold and _mt <= 2)):
                continue
            REACHABLE_W8.add((_mt, 3, _ntb, _fold))
        REACHABLE_W8.add((_mt, 5, 1, _fold))
        if _mt <= 2:
            REACHABLE_W8.add((_mt, 5, 2, _fold))


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)


def form_key(nat, dtype, M, N, K, rpw=0, fold=False):
    p = nat.skinny_plan_w8(dtype, M, N, K, rpw, fold)
    return (p["row_tiles_per_wg"], 3 if p["ksteps_per_wave"] <= 3 else 5, p["tiles_per_wg"], bool(fold))


_W = {}


def weights(nat, K, N, seed):
    """(original fp64 [K, N], codes uint8, scale fp32, dequantised fp64, packed image), cached: computed once per shape."""
    if (K, N, seed) not in _W:
        from indextts.utils import quant
        w = rnd(K, N, seed=seed + 1, device=DEV) / math.sqrt(K) * (0.25 + 4.0 * torch.rand(N, generator=torch.Generator().manual_seed(seed)).double().to(DEV))
        codes, scale = quant.quantize_e4m3_cols(w)
        _W[(K, N, seed)] = (w, codes, scale.contiguous(), quant.dequantize(codes, scale), nat.pack_weight_w8(codes))
    return _W[(K, N, seed)]


def np_pack(codes, K, N):
    """The documented layout, restated: block (nt, kb) at ((nt * KB + kb) * 1024); lane (g, c) owns 16 bytes, byte e < 8 = code[kb * 64 +
    g * 8 + e][nt * 16 + c], byte 8 + e = code[kb * 64 + 32 + g * 8 + e][nt * 16 + c]; zero padding."""
    NT, KB = -(-N // 16), -(-K // 64)
    pad = np.zeros((KB * 64, NT * 16), dtype=np.uint8)
    pad[:K, :N] = codes
    out = np.zeros((NT, KB, 4, 16, 16), dtype=np.uint8)          # [nt][kb][g][c][byte]
    for nt in range(NT):
        for kb in range(KB):
            for g in range(4):
                for half in range(2):
                    rows = pad[kb * 64 + half * 32 + g * 8: kb * 64 + half * 32 + g * 8 + 8, nt * 16: nt * 16 + 16]   # [e][c]
                    out[nt, kb, g, :, half * 8: half * 8 + 8] = rows.T
    return out.reshape(-1)


@pytest.mark.parametrize("K,N", [(96, 20), (128, 32)])
def test_pack_matches_the_documented_layout(nat, K, N):
    codes = torch.from_numpy(np.random.default_rng(K).integers(0, 255, size=(K, N)).astype(np.uint8))
    got = nat.pack_weight_w8(codes.to(DEV)).cpu().numpy()
    want = np_pack(codes.numpy(), K, N)
    assert got.shape == want.shape == (-(-N // 16) * -(-K // 64) * 1024,)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
def test_every_code_decodes_exactly(nat, dtype):
    """All 254 non-NaN codes, scale 1, one-hot rows of x: every output IS the decoded value (subnormals included), bit for bit."""
    from indextts.utils import quant
    allc = [c for c in range(256) if c & 0x7f != 0x7f]
    K, N, M = 256, 20, 96
    codes = torch.zeros(K, N, dtype=torch.uint8)
    for n in range(N):                                            # every column holds every code, at another k
        codes[:254, n] = torch.tensor([allc[(k + 17 * n) % 254] for k in range(254)], dtype=torch.uint8)
    want = quant.decode_e4m3(codes).float().to(DEV)
    wp = nat.pack_weight_w8(codes.to(DEV))
    one = torch.ones(N, dtype=torch.float32, device=DEV)
    for j in range(3):
        ks = torch.arange(96 * j, 96 * j + M)
        x = torch.zeros(M, K, dtype=dtype, device=DEV)
        live = ks < K
        x[torch.arange(M)[live], ks[live]] = 1.0
        for packed in (False, True):
            yf = torch.full((M, N), 7.0, device=DEV)
            nat.gemm_skinny_w8(dtype, M, N, K, wp, one, None, x=nat.pack_activation(x) if packed else x, x_packed=packed,
                               epi=nat.EPI_STORE_F32, yf=yf)
            ref = torch.zeros(M, N, device=DEV)
            ref[live.to(DEV)] = want[ks[live].to(DEV)]
            assert torch.equal(yf, ref), f"{tname(dtype)} launch {j} packed={packed}: {(yf != ref).sum().item()} outputs differ from the decoded codes"


def run_w8(nat, dtype, M, N, K, epi, fold=False, rpw=0, ypk=False, bs=0, controls=False, seed=0):
    """One itts_gemm_skinny_w8 launch (row-major and packed x: equal bits) against the fp64 reference over the dequantised weights."""
    key = form_key(nat, dtype, M, N, K, rpw, fold)
    what = f"w8 {tname(dtype)} {key} M={M} N={N} K={K} {epi}" + (f" rows_per_wg={rpw}" if rpw else "") + (" packed-y" if ypk else "") + \
        (f" paged{bs}" if bs else "")
    x = (fold_rows(M, K, seed, DEV) if fold else rnd(M, K, seed=seed, device=DEV)).to(dtype)
    w0, codes, scale, w, wp = weights(nat, K, N, seed)
    bias = rnd(N, seed=seed + 2, device=DEV).float()
    bias[-1] = 0.75
    fo, kw = None, dict(rows_per_wg=rpw)
    if fold:
        fo = (w.sum(0).float().contiguous(), bias, 1e-5)        # ln_c = w_scale . sum_k decode, summed in float64
        kw.update(ln_c=fo[0], ln_eps=1e-5)
    mtp = (M + 15) // 16
    xp = nat.pack_activation(x)
    lim = lambda ref, S, extra, L=None: (ulp(ref, dtype) + (L or 1.0) * (2.0 ** -21 * S + extra) + (2.0 ** -21 * ref.abs() if L else 0.0))  # noqa: E731
    f32lim = lambda S, extra: 2.0 ** -21 * S + extra + 1e-300  # noqa: E731

    def both(make_out, names, **okw):
        o1, o2 = make_out(), make_out()
        for xa, packed, o in ((x, False, o1), (xp, True, o2)):
            nat.gemm_skinny_w8(dtype, M, N, K, wp, scale, bias, x=xa, x_packed=packed, **kw, **dict(zip(names, o)), **okw)
        for a, b in zip(o1, o2):
            assert torch.equal(a, b), f"{what}: packed and row-major x differ"
        return o1

    if epi in ("store", "gelu"):
        f, L = (gelu_new, 1.13) if epi == "gelu" else ((lambda v: v), None)
        mk = (lambda: (torch.full((mtp * 16 * N,), 7.0, dtype=dtype, device=DEV),)) if ypk else \
            (lambda: (torch.full((M, N), 7.0, dtype=dtype, device=DEV),))
        (y,) = both(mk, ("y",), epi=nat.EPI_GELU_STORE if epi == "gelu" else nat.EPI_STORE, y_packed=ypk)
        got = nat.unpack_activation(y, mtp * 16, N)[:M] if ypk else y

        def ref_of(w_, fo_):
            pre, S, extra = gemm_pre(x, w_, bias, fo_)
            r = f(pre)
            return r, lim(r, S, extra, L)
    elif epi == "store_f32":
        (got,) = both(lambda: (torch.full((M, N), 7.0, device=DEV),), ("yf",), epi=nat.EPI_STORE_F32)

        def ref_of(w_, fo_):
            pre, S, extra = gemm_pre(x, w_, bias, fo_)
            return pre, f32lim(S, extra)
    elif epi == "resid":
        h0 = rnd(M, N, seed=seed + 3, scale=2.0, device=DEV).float()
        mk = lambda: (h0.clone(), torch.full((mtp * 16 * N,) if ypk else (M, N), 7.0, dtype=dtype, device=DEV))  # noqa: E731
        got, ycopy = both(mk, ("yf", "y"), epi=nat.EPI_RESID_F32, y_packed=ypk)
        full = nat.unpack_activation(ycopy, mtp * 16, N) if ypk else ycopy
        assert torch.equal(full[:M], got.to(dtype)), f"{what}: the T copy is not the rounded fp32 row"

        def ref_of(w_, fo_):
            pre, S, extra = gemm_pre(x, w_, bias, fo_)
            return pre + h0.double(), f32lim(S + h0.double().abs(), extra)
    elif epi == "qkv":
        H = N // 192
        D, pos = H * 64, 37
        posd = i32([pos])
        if bs:                                                    # a two-block table: the block of *pos and the one behind it
            e = (pos // bs) % TAB
            tab = np.zeros((M, TAB), dtype=np.int32)
            blocks = np.random.default_rng(seed).permutation(np.arange(1, 1 + 2 * M)).reshape(M, 2)
            tab[:, e], tab[:, (e + 1) % TAB] = blocks[:, 0], blocks[:, 1]
            mk = lambda: (torch.full((M, D), 7.0, dtype=dtype, device=DEV),  # noqa: E731
                          torch.full((1 + 2 * M, H, bs, 64), 7.0, dtype=dtype, device=DEV),
                          torch.full((1 + 2 * M, H, bs, 64), 7.0, dtype=dtype, device=DEV))
            okw = dict(epi=nat.EPI_QKV_CACHE, pos=posd, heads=H, smax=0, kv_tab=i32(tab), kv_bs=bs)
        else:
            smax = 48
            mk = lambda: (torch.full((M, D), 7.0, dtype=dtype, device=DEV),  # noqa: E731
                          torch.full((M, H, smax, 64), 7.0, dtype=dtype, device=DEV),
                          torch.full((M, H, smax, 64), 7.0, dtype=dtype, device=DEV))
            okw = dict(epi=nat.EPI_QKV_CACHE, pos=posd, heads=H, smax=smax)
        q, kc, vc = both(mk, ("y", "kcache", "vcache"), **okw)

        def appended(cache):
            if bs:
                return cache[torch.from_numpy(tab[:, e].astype(np.int64)).to(DEV), :, pos % bs].reshape(M, D)
            return cache[:, :, pos].reshape(M, D)
        for cache in (kc, vc):
            t = cache.clone()
            if bs:
                t[torch.from_numpy(tab[:, e].astype(np.int64)).to(DEV), :, pos % bs] = 7.0
            else:
                t[:, :, pos] = 7.0
            assert (t == 7.0).all(), f"{what}: a cache position other than *pos was written"
        got = torch.cat([q, appended(kc), appended(vc)], 1)

        def ref_of(w_, fo_):
            pre, S, extra = gemm_pre(x, w_, bias, fo_)
            return pre, lim(pre, S, extra)
    else:
        raise AssertionError(epi)

    ref, bound = ref_of(w, fo)
    ok(what, got, ref, bound)
    if controls:
        from indextts.utils import quant
        wd = w.clone()
        wd[:, 1] = quant.decode_e4m3(codes)[:, 1]
        bad(what, "the scale of column 1 dropped", got, ref_of(wd, fo)[0], bound)
        wh = w.clone()
        wh[0:32], wh[32:64] = w[32:64], w[0:32]
        bad(what, "the two 32-k halves of block 0 swapped", got, ref_of(wh, fo)[0], bound)
        if fold:
            bad(what, "ln_c from the unquantised gamma . W", got, ref_of(w, (w0.sum(0).float(), bias, 1e-5))[0], bound)
    return key


MS, KS_ = (1, 16, 33, 96), (64, 96, 1280)
# epilogue family -> (epi, N list, options); each N at every M and K
FAMILIES = {
    "store": ("store", (16, 20), {}),
    "store-packed-y": ("store", (64,), dict(ypk=True)),
    "qkv": ("qkv", (192,), {}),
    "qkv-paged": ("qkv", (192,), dict(bs=16)),
    "gelu": ("gelu", (16, 20), {}),
    "resid": ("resid", (16, 20), {}),
    "resid-packed-hb": ("resid", (64,), dict(ypk=True)),
    "store_f32": ("store_f32", (16, 20, 50), {}),
}
CROSS = [(fam, fold) for fam in FAMILIES for fold in (False, True) if not (fold and fam.startswith("resid"))]   # (no folded residual form)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("fam,fold", CROSS, ids=lambda v: v if isinstance(v, str) else ("fold" if v else "plain"))
def test_w8_forms_fp64(nat, dtype, fam, fold):
    epi, Ns, opt = FAMILIES[fam]      # (negative controls: once per family, at 96 rows -- every class of fold_rows -- and K = 1280)
    for N in Ns:
        if fold and N % 4:
            continue                                              # the folded form needs N % 4 == 0 (refused otherwise)
        for K in KS_:
            for M in MS:
                run_w8(nat, dtype, M, N, K, epi, fold=fold, controls=(N == Ns[0] and K == 1280 and M == 96), seed=M + K, **opt)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
def test_every_built_form(nat, dtype):
    """Every instantiation of the W8 family runs once against the fp64 reference: shapes are searched with the planner (wide N for
    2-4 column tiles per workgroup, K = 1664 for 5 blocks per pass, rows dealt to grid.z), and the forms found must be the list."""
    found = {}
    cands = [(M, rpw, N, K) for K in (96, 1664) for N in (64, 2064, 4112, 8196) for M, rpw in
             ((16, 0), (32, 0), (33, 0), (96, 0), (96, 16), (80, 16), (96, 32))]
    for fold in (False, True):
        for M, rpw, N, K in cands:
            k = form_key(nat, dtype, M, N, K, rpw, fold)
            found.setdefault(k, (M, N, K, rpw, fold))
    assert set(found) == REACHABLE_W8, (sorted(REACHABLE_W8 - set(found)), sorted(set(found) - REACHABLE_W8))
    epis = ("store", "gelu", "store_f32", "resid")
    for i, (k, (M, N, K, rpw, fold)) in enumerate(sorted(found.items())):
        epi = epis[i % (3 if fold else 4)]
        assert run_w8(nat, dtype, M, N, K, epi, fold=fold, rpw=rpw, seed=i) == k
    _W.clear()


# More than 96 rows through the entry point: without rows_per_wg it walks the rows 96 at a time (the last chunk plans for its own row
# count), with rows_per_wg 16 / 32 every row tile goes to grid.z of ONE launch.  (M, N, K, epilogue, options)
MANY_ROWS = [
    (97, 20, 96, "store", {}),                                    # 96 rows, then 1
    (130, 64, 1280, "resid", dict(ypk=True)),                     # 96, then 34 (4 row tiles, the last two ragged / empty), packed copy
    (130, 192, 96, "qkv", dict(bs=16, fold=True)),                # the KV append of the second chunk lands in ITS rows' blocks
    (200, 64, 1280, "gelu", dict(rpw=16, fold=True, ypk=True)),   # 13 row tiles dealt to grid.z
    (200, 50, 96, "store_f32", dict(rpw=32)),                     # 7 workgroup rows of 2 tiles, the last half empty
    (256, 192, 1280, "qkv", dict(rpw=32, fold=True)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
def test_more_than_96_rows(nat, dtype):
    for i, (M, N, K, epi, opt) in enumerate(MANY_ROWS):
        run_w8(nat, dtype, M, N, K, epi, seed=40 + i, **opt)


def test_unsupported_forms_are_refused(nat):
    x = torch.zeros(4, 64, dtype=BF16, device=DEV)
    w = nat.pack_weight_w8(torch.zeros(64, 64, dtype=torch.uint8, device=DEV))
    s = torch.ones(64, device=DEV)
    y = torch.zeros(4, 64, dtype=BF16, device=DEV)
    with pytest.raises(nat.NativeError, match="itts_gemm_skinny_w8: ksplit"):
        nat.gemm_skinny_w8(BF16, 4, 64, 64, w, s, x=x, y=y, ksplit=2)
    with pytest.raises(nat.NativeError, match="itts_gemm_skinny_w8: the activation type"):
        nat.gemm_skinny_w8(torch.float32, 4, 64, 64, w, s, x=x.float(), y=y.float())
    with pytest.raises(nat.NativeError, match="itts_gemm_skinny_w8: epilogue"):
        nat.gemm_skinny_w8(BF16, 4, 64, 64, w, s, x=x, y=y, epi=nat.EPI_RELU_AFFINE_STORE)
