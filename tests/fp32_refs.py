"""float64 references of the fp32 forms of the GPT half -- itts_gemm_skinny, itts_attn_decode, the four prefill attention entry points,
itts_ln_reduce / itts_layernorm and itts_kv_share_rows --, their per-element bounds, their negative controls, the operand generators
and the case lists of tests/test_fp32_kernels_gpu.py.  Device-agnostic plain torch: every function works on the device of its operands
and makes no call into the library, so tests/test_fp32_refs_cpu.py can hold each reference to torch's own float64 operators, let a
plain float32 evaluation stand in for the kernel and show that every control leaves its bound, without a GPU.

Skinny GEMM (Elem<float>: k-steps of KS = 16, one k-step = four v_mfma_f32_16x16x4_f32; MT = 1, rows cut 16 at a time by the entry
point).  With S = sum_k |x w| + |bias| (+ |resid|):
      STORE, STORE_F32, QKV_CACHE, RESID_F32, SLAB_F32      |y - ref| <= ulp_f32(ref) + CHAIN S           CHAIN = 2^-21
      GELU_STORE                                            |y - ref| <= ulp_f32(ref) + 1.13 CHAIN S + G32(pre)
  CHAIN is the project's fp32-chain figure and G32 the activation's own fp32 error, both taken unchanged from
  tests/plain_gemm_refs.py (which applies them to its fp32 cases); a slab is held to the S of its own K slice: k-steps
  [s SB, min((s + 1) SB, KT)) with SB = ceil(KT / ksplit), the bias in slab 0.  Nothing is re-derived: at K = 5120 a wave adds 40
  k-steps in four register passes, eight waves are summed in a fixed order through LDS, and 2^-21 S = 8 u S stays far above what that
  chain loses on operands whose partial sums grow like sqrt(k) while S grows like k (profiles/fp32_kernels_fp64.txt has the ratios).

Decode attention (attn_decode_kernel<float, 4, ...>: E = 4 dims per lane, LPR = 16 lanes per key row, RPW = 4 rows per wave-load, a
pass is 4 waves x 8 chunks x 4 rows = 128 keys and is never context-sized; key groups are cut from pad & ~3).  With p_j the softmax
weights of the visible keys and A = sum_j p_j |v_j|:
      bound = ulp_f32(ref) + C_ATTN A,      C_ATTN = 2^-16
  The 16-bit file's budget restated for these counts (u = 2^-24): a score is E = 4 fmaf per lane and log2 LPR = 4 shuffle additions,
  |ds| <= 8 u sum |q k| / 8 (about 10 for these inputs: 80 u; 16-bit: 11 chained operations, 110 u); __expf is unchanged, 19 u; the
  sums l and o take at most 8 additions per lane and pass (4 passes at 385 slots: 32), log2 RPW = 2 shuffle merges inside a wave
  (16-bit: 3) and the 4-wave LDS merge: 40 u as before.  Per weight about 140 u relative instead of 170 u, |out - ref| <= 2 * 140 u A
  = 2^-15.9 A if every rounding pushed the same way: the restated worst case is 1.07 x the cap of 2^-16, not below it, so the file's
  constant stands (the independent roundings again sum to about 25 u A).
  Inputs put weight on the boundary keys: scores have a standard deviation of 2, and the first visible key, the key in front of it,
  the key at *pos, the first key of every 32-key quarter and with it of every 128-key pass are given a score of 6.

Prefill attention (attn_prefill_kernel<float>: exact-fp32 MFMA, P is not rounded before P V): a plain float64 softmax over the
visible keys, and the fp32-level part of the 16-bit file's bound,
      bound = ulp_f32(ref) + sum_j p_j delta_j |v_j| + |ref| sum_j p_j delta_j,      delta_j = 2^-21 (T_j + T_max) + 2^-19
  with p_j the normalised weights, T_j = sum_d |q_d k_jd| / 8 and T_max its maximum over the row's visible keys.

LayerNorm (ln_reduce_kernel / layernorm_kernel, fp32 output): `ln_ref`, the 16-bit file's reference and budget E (C_LN = 2^-20),
plus ulp_f32(ref); h after the slab sum is the fixed-order fp32 sum bit for bit (`slab_sum`).

itts_kv_share_rows moves bytes: `kv_share_expected` is the cache after the copy, compared with ==.

Negative controls: each re-evaluates a reference with one thing wrong (GEMM_CONTROLS, `decode_controls`, the prefill arguments `drop` /
`causal_shift` / `lo`, ln_ref's `cols` / `eps`); the kernel's output is compared with it under the same bound and must fail."""
import math

import numpy as np
import torch

from fp64_check import rnd, ulp
from plain_gemm_refs import CHAIN, L_GELU, gelu_f32_term, gelu_new

F32 = torch.float32
KS = 16                 # k-step of the fp32 MFMA form
TAB = 64                # ITTS_KV_TAB: entries of a row's block table
C_ATTN = 2.0 ** -16
C_LN = 2.0 ** -20
RPW, PASS = 4, 128      # rows per wave-load and keys per pass of attn_decode_kernel<float, 4, ...>


# ----------------------------------------------------------------------------------------------------------- skinny GEMM
GEMM_CONTROLS = {
    "drop_last_kstep": "the last k-step dropped",
    "swap_wtiles": "the first two 16-column weight tiles exchanged",
    "rows16_shift": "rows 16.. shifted by one (row i reads x[i - 1])",
}
SLAB_MISSING = "one slab missing"
EPIS = ("store", "gelu", "qkv", "resid", "slab", "store_f32")

P = lambda **kw: kw  # noqa: E731
# (M, N, K, form key, options).  N = "N2" / "N3": the smallest N at which skinny_plan returns 2 / 3 column tiles per workgroup of the
# SPW 5 form (the test reads them from the planner at K = 16; the 10-step form stops at 2 tiles).  M = 17 and 33 make the entry point
# launch twice / three times: the second chunk's x, y, yf, cache rows, table rows and slab rows are what those cases are about.
GEMM_CASES = [
    # ---- the K walk: 1 step (one wave); 6; 40 | 41 (SPW 5 -> 10); 80 (one full pass); 81 (a second pass of one step); 320 (four passes)
    (1, 50, 16, (1, 5, 1, False, 8), P(epi="store_f32", controls=True)),
    (13, 64, 96, (1, 5, 1, False, 8), P(epi="store", ypk=True)),
    (16, 64, 640, (1, 5, 1, False, 8), P(epi="gelu")),
    (16, 50, 656, (1, 10, 1, False, 8), P(epi="store_f32")),
    (32, 64, 1280, (1, 10, 1, False, 8), P(epi="gelu", ypk=True)),
    (33, 64, 1296, (1, 10, 1, False, 8), P(epi="store", ypk=True, y_row0=16, controls=True)),
    (32, 50, 5120, (1, 10, 1, False, 8), P(epi="store_f32")),
    (17, 64, 5120, (1, 10, 1, False, 8), P(epi="resid", ypk=True, y_row0=16)),
    # ---- 16 waves: more than 80 k-steps in the slice (81: one wave-step each and a remainder; 320: two passes of the 16-wave form)
    (13, 64, 1296, (1, 10, 1, False, 16), P(epi="resid", wide=True)),
    (17, 50, 5120, (1, 10, 1, False, 16), P(epi="store_f32", wide=True, controls=True)),
    # ---- column tiles per workgroup, from the planner
    (16, "N2", 96, (1, 5, 2, False, 8), P(epi="store_f32")),
    (17, "N3", 96, (1, 5, 3, False, 8), P(epi="gelu")),
    (13, "N2", 656, (1, 10, 2, False, 8), P(epi="store")),
    (5, "N3", 5120, (1, 10, 2, False, 8), P(epi="store_f32")),
    # ---- the residual epilogue: resid aliases yf, with and without the T-typed copy
    (17, 64, 1280, (1, 10, 1, False, 8), P(epi="resid", controls=True)),
    (33, 64, 96, (1, 5, 1, False, 8), P(epi="resid", copy=False)),
    # ---- QKV + cache append: contiguous rows, paged pool (16 and 64 positions per block)
    (13, 384, 16, (1, 5, 1, False, 8), P(epi="qkv", controls=True)),
    (17, 384, 1280, (1, 10, 1, False, 8), P(epi="qkv", controls=True)),
    (33, 384, 96, (1, 5, 1, False, 8), P(epi="qkv", bs=16, controls=True)),
    (17, 384, 656, (1, 10, 1, False, 8), P(epi="qkv", bs=64)),
    # ---- split-K slabs: 5 k-steps in 2 slices (3 + 2), 7 in 3 (3 + 3 + 1: a one-step slice), 320 in 3 (107 + 107 + 106)
    (13, 50, 80, (1, 5, 1, False, 8), P(epi="slab", ksplit=2, controls=True)),
    (33, 64, 112, (1, 5, 1, False, 8), P(epi="slab", ksplit=3, controls=True)),
    (17, 64, 5120, (1, 10, 1, False, 8), P(epi="slab", ksplit=3)),
    (1, 64, 1280, (1, 5, 1, False, 8), P(epi="slab", ksplit=2)),         # 40 k-steps per slice: 5 per wave, one pass of the SPW 5 form
]


def slices(K, ksplit):
    """Column ranges [k0, k1) of the split-K slices: SB = ceil(KT / ksplit) k-steps each, the last takes what is left."""
    KT = K // KS
    SB = -(-KT // ksplit)
    return [(min(s * SB, KT) * KS, min((s + 1) * SB, KT) * KS) for s in range(ksplit)]


def gemm_operands(M, N, K, seed, device="cpu"):
    """x [M][K], w [K][N], bias [N], h0 [M][N] (the residual stream RESID_F32 adds into): drawn in float64, rounded to fp32."""
    x = rnd(M, K, seed=seed, device=device).float()
    w = (rnd(K, N, seed=seed + 1, device=device) / math.sqrt(K)).float()
    bias = rnd(N, seed=seed + 2, device=device).float()
    bias[-1] = 0.75
    h0 = rnd(M, N, seed=seed + 3, scale=2.0, device=device).float()
    return x, w, bias, h0


def gemm_ref(x, w, bias, epi="store", resid=None, ksplit=1, ctl=None):
    """(ref, bound) float64 of one itts_gemm_skinny call on fp32 operands; `slab`: [ksplit][M][N], each slab on its own K slice.
    ctl: one of GEMM_CONTROLS, evaluated wrong in that one way."""
    assert epi in EPIS and (ctl is None or ctl in GEMM_CONTROLS)
    xd, wd = x.double(), w.double()
    M, K = xd.shape
    if ctl == "drop_last_kstep":
        wd = wd.clone()
        wd[K - KS:] = 0
    if ctl == "swap_wtiles":
        wd = torch.cat([wd[:, 16:32], wd[:, :16], wd[:, 32:]], 1)
    if ctl == "rows16_shift":
        assert M > 16
        xd = torch.cat([xd[:16], xd[15:M - 1]])
    bd = None if bias is None else bias.double()
    if epi == "slab":
        refs, mags = [], []
        for s, (k0, k1) in enumerate(slices(K, ksplit)):
            acc, mag = xd[:, k0:k1] @ wd[k0:k1], xd[:, k0:k1].abs() @ wd[k0:k1].abs()
            if s == 0 and bd is not None:
                acc, mag = acc + bd, mag + bd.abs()
            refs.append(acc)
            mags.append(mag)
        ref, S = torch.stack(refs), torch.stack(mags)
        return ref, ulp(ref, F32) + CHAIN * S
    assert ksplit == 1
    pre, S = xd @ wd, xd.abs() @ wd.abs()
    if bd is not None:
        pre, S = pre + bd, S + bd.abs()
    if epi == "gelu":
        ref = gelu_new(pre)
        return ref, ulp(ref, F32) + L_GELU * CHAIN * S + gelu_f32_term(pre)
    if epi == "resid":
        pre, S = pre + resid.double(), S + resid.double().abs()
    return pre, ulp(pre, F32) + CHAIN * S


# ----------------------------------------------------------------------------------------------------------- decode attention
# (pos, pads): one launch per residue of the context mod 4 (slots = pos + 1 - (pad & ~3) is congruent to the context).  The last row of
# every launch is skipped and must keep its sentinel.  pads[0] is small: the shared forms read row 0's positions [pads[0], pads[0] + C).
DECODE_LAUNCHES = [
    (388, [5, 388, 385, 262, 135, 0, 1, 2, 3, 70, 21]),      # slots 385, 1, 5, 129, 257, 389 x 4, 321
    (130, [6, 129, 0, 3, 70, 44]),                           # slots 127, 3, 131, 131, 63
    (259, [7, 257, 133, 0, 2, 90]),                          # slots 256, 4, 128, 260, 260
]
DECODE_SLOTS = {1, 3, 4, 5, 127, 128, 129, 256, 257, 385}
DECODE_PADS = {0, 1, 2, 3, 5, 70}
DECODE_FORMS = ["contiguous", "packed-out", "paged16", "paged16-packed-out", "paged32-packed-out", "paged64", "row-table", "row-table-packed-out",
                "share", "paged16-share"]
SHARE_C = 19


def decode_slots(pos, pad):
    return pos + 1 - (pad & ~(RPW - 1))


def decode_case(pads, pos, H, seed, device="cpu", same_q=False):
    """q [B][H][64] and logical caches k, v [B][H][smax][64] (fp32) with weight on the boundary keys (module docstring)."""
    B, smax = len(pads), pos + 9
    q = (rnd(B, H, 64, seed=seed, device=device) * 2.0).float()
    if same_q:      # shared first keys: one query for every row, so that row 0's boundary keys carry weight in the rows they are read for
        q = q[0:1].expand(B, H, 64).contiguous()
    k = rnd(B, H, smax, 64, seed=seed + 1, device=device)
    v = rnd(B, H, smax, 64, seed=seed + 2, device=device).float()
    qd = q.double()
    boost = 8.0 * 6.0 * qd / (qd * qd).sum(-1, keepdim=True)       # a key with score 6: three standard deviations up
    for b, p in enumerate(pads):
        b0 = p & ~(RPW - 1)
        marks = {p, max(p - 1, 0), pos} | set(range(b0 + PASS // 4, pos + 1, PASS // 4))
        for j in marks:
            k[b, :, j] = boost[b]
    return q, k.float(), v, smax


def decode_ref(q, k, v, pads, pos, lo_shift=0, drop=None):
    """fp64 softmax(q k / 8) v over the keys [pad_b + lo_shift, pos] of every row, minus the key drop[b]; returns (ref, A), [B][H * 64]."""
    B, H, smax, _ = k.shape
    dev = k.device
    s = torch.einsum("bhd,bhjd->bhj", q.double(), k.double()) * 0.125
    j = torch.arange(smax, device=dev)[None, :]
    lo = torch.tensor(pads, device=dev)[:, None] + lo_shift
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


def decode_bound(ref, A):
    return ulp(ref, F32) + C_ATTN * A


def decode_controls(q, k, v, pads, pos):
    """{description: wrong reference} of the controls every decode form shares.  A control that leaves a row without any key gives
    NaN there: the caller masks those rows."""
    b0s = [p & ~(RPW - 1) for p in pads]
    return {
        "the key at pad[b] - 1 let in": decode_ref(q, k, v, pads, pos, lo_shift=-1)[0],
        "the key at pad[b] left out": decode_ref(q, k, v, pads, pos, lo_shift=1)[0],
        "the key at *pos left out": decode_ref(q, k, v, pads, pos, drop=[pos if p < pos else None for p in pads])[0],
        "the first key of the second pass left out": decode_ref(q, k, v, pads, pos, drop=[b0 + PASS if b0 + PASS <= pos else None for b0 in b0s])[0],
    }


def paged_pool(k, v, bs, seed, fill=0.0):
    """Logical caches [B][H][smax][64] dealt into a shuffled block pool [1 + B nb][H][bs][64] behind a 64-entry table; block 0 is the
    scratch block every unmapped entry names."""
    B, H, smax, _ = k.shape
    nb = (smax + bs - 1) // bs
    assert nb <= TAB - 2
    tab = np.zeros((B, TAB), dtype=np.int32)
    tab[:, :nb] = np.random.default_rng(seed).permutation(np.arange(1, 1 + B * nb)).reshape(B, nb)
    idx = torch.from_numpy(tab[:, :nb].astype(np.int64)).to(k.device)
    pk = torch.full((1 + B * nb, H, bs, 64), fill, dtype=k.dtype, device=k.device)
    pv = torch.full_like(pk, fill)
    pad_to = nb * bs - smax
    kk = torch.nn.functional.pad(k, (0, 0, 0, pad_to), value=fill).view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4)
    vv = torch.nn.functional.pad(v, (0, 0, 0, pad_to), value=fill).view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4)
    pk[idx], pv[idx] = kk, vv
    return pk, pv, tab


def unpage(pool, tab, smax, bs):
    """Logical [B][H][smax][64] view of a pool through a (possibly altered) table: what a reference with that table reads."""
    nb = (smax + bs - 1) // bs
    idx = torch.from_numpy(tab[:, :nb].astype(np.int64)).to(pool.device)
    t = pool[idx].permute(0, 2, 1, 3, 4)
    return t.reshape(t.shape[0], t.shape[1], nb * bs, 64)[:, :, :smax]


# ----------------------------------------------------------------------------------------------------------- prefill attention
def prefill_ref(q, k, v, qpos, lo, drop=None, causal_shift=0):
    """fp64 attention of queries q [Q][H][64] at sequence positions qpos [Q] over keys k / v [J][H][64]: key j visible iff
    lo <= j <= qpos + causal_shift (and j not in drop).  Returns (ref [Q][H * 64], bound, visible count [Q]); rows without a key: zeros."""
    Q, H, _ = q.shape
    J = k.shape[0]
    dev = q.device
    s = torch.einsum("qhd,jhd->hqj", q.double(), k.double()) * 0.125
    T = torch.einsum("qhd,jhd->hqj", q.double().abs(), k.double().abs()) * 0.125
    j = torch.arange(J, device=dev)[None, :]
    vis = (j >= lo) & (j <= (qpos[:, None] + causal_shift))
    if drop is not None:
        vis[:, drop] = False
    s = s.masked_fill(~vis[None], -math.inf)
    T = T * vis[None]
    delta = 2.0 ** -21 * (T + T.max(-1, keepdim=True).values) + 2.0 ** -19
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    p = p / torch.clamp(l, min=1e-300)
    vd = v.double().transpose(0, 1)                               # [H][J][64]
    out = lambda t: t.transpose(0, 1).reshape(Q, H * 64)  # noqa: E731
    ref = out(p @ vd)
    E = out((p * delta) @ vd.abs()) + out((p * delta).sum(-1, keepdim=True).expand(H, Q, 64)) * ref.abs()
    return ref, ulp(ref, F32) + E, vis.sum(-1)


def split_qkv(qkv, H):
    D = H * 64
    return tuple(t.reshape(-1, H, 64) for t in qkv.split(D, dim=-1))


def prefill_inputs(rows, H, seed, device="cpu"):
    """qkv [rows][3 H 64] fp32; q scaled so that scores have a standard deviation of 2."""
    D = H * 64
    t = rnd(rows, 3 * D, seed=seed, device=device)
    t[:, :D] *= 2.0
    return t.float()


# ----------------------------------------------------------------------------------------------------------- row kernels
def ln_ref(x, w, b, eps=1e-5, cols=None, e_in=None):
    """fp64 LayerNorm of the rows x [M][D] (statistics over the first `cols` columns: all by default) and its fp32-level budget E,
    as derived in tests/test_decode_kernels_gpu.py (ln_ref there): the two-pass statistics of ln_math.h with centred squares,
        |y - ref| <= C_LN |ref - b| + 2^-21 |w| rstd E|x| + 2^-24 |ref|,     C_LN = 2^-20.
    e_in (second LayerNorm of a pair): per-element error bound of x itself, carried through as |w| rstd (e_i + mean e + |n_i| rms e)."""
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


def ln_pair(h, lw, lb, lw2=None, lb2=None, eps=1e-5, cols=None):
    """(ref, bound) of LN(h) or LN2(LN(h)) into an fp32 output."""
    ref, E = ln_ref(h, lw, lb, eps, cols)
    if lw2 is not None:
        ref, E = ln_ref(ref, lw2, lb2, eps, cols, e_in=E)
    return ref, ulp(ref, F32) + E


def fma32(t, b, v):
    """fmaf(t, b, v) of fp32 tensors: the product of two fp32 values is exact in float64."""
    return (t.double() * b.double() + v.double()).float()


def slab_sum(h0, slab, slabs, D, bias=None, lora_b=None):
    """h after itts_ln_reduce's update, in the kernel's order and in fp32: h0 + bias + slab[0] + slab[1] + ... over the slab indices
    `slabs`, then for every LoRA rank j one fmaf of the slabs' summed column D + j with lora_b[j].  No slabs: h0 itself."""
    v = h0.clone()
    if not slabs:
        return v
    if bias is not None:
        v = v + bias
    for i in slabs:
        v = v + slab[i][:, :D]
    if lora_b is not None:
        for j in range(lora_b.shape[0]):
            t = torch.zeros(h0.shape[0], device=h0.device)
            for i in slabs:
                t = t + slab[i][:, D + j]
            v = fma32(t[:, None], lora_b[j][None, :], v)
    return v


def ln_reduce_configs(M, ypk):
    """(D, nslab, bias, LoRA rank, second LayerNorm) of test_ln_reduce_fp64, the 16-bit file's list."""
    r = {1: 4, 13: 16, 32: 24, 96: 16}[M]
    configs = [(1280, 0, False, 0, False), (1280, 3, True, r, False), (1280, 6, True, 0, True), (1280, 3, False, 0, True), (256, 6, True, r, True)]
    if not ypk:
        configs.append((320, 3, True, 0, True))
    return configs


def ln_reduce_operands(M, D, nslab, has_bias, lr, two, seed, device="cpu"):
    """Operands of one ln_reduce configuration, as the 16-bit test draws them: row 0 has a small variance (sigma 0.01: eps matters)."""
    stride = D + 16 * ((lr + 15) // 16) if lr else (D + 64 if (nslab == 6 and D == 1280) else D)
    g = lambda *s, seed, scale=1.0: rnd(*s, seed=seed, scale=scale, device=device)  # noqa: E731
    h0 = (g(M, D, seed=seed, scale=2.0) + 0.3).float()
    h0[0] = (g(D, seed=seed + 1) * 0.01 + 0.5).float()
    slab = g(max(nslab, 1), M, stride, seed=seed + 2, scale=0.5 if M > 1 or nslab == 0 else 0.001).float()
    if nslab:
        slab[:, 0] *= 0.002        # row 0 keeps its small variance through the update
    bias = (g(D, seed=seed + 3) * 0.001).float() if has_bias else None
    lw, lb = (1 + 0.1 * g(D, seed=seed + 4)).float(), (0.1 * g(D, seed=seed + 5)).float()
    lw2, lb2 = ((1 + 0.1 * g(D, seed=seed + 6)).float(), (0.1 * g(D, seed=seed + 7)).float()) if two else (None, None)
    lora_b = (g(lr, D, seed=seed + 8) * 0.05).float() if lr else None
    return dict(h0=h0, slab=slab, bias=bias, lw=lw, lb=lb, lw2=lw2, lb2=lb2, lora_b=lora_b, stride=stride)


# ----------------------------------------------------------------------------------------------------------- the cache copy
KVS = dict(L=2, B=3, H=2, p0=29, pads=[4, 14, 45], smax=80, bs=16)      # p0 differs from every pad; [29, 34), [14, 19) and [45, 50) straddle a block


def kv_share_expected(cache, B, C, p0, pads):
    """Logical caches [L][rows][H][smax][64] after itts_kv_share_rows: row b's positions [pad_b, pad_b + C) hold row 0's [p0, p0 + C)
    for b = 1 .. B - 1, everything else (row 0, rows >= B, every other position) what it held."""
    want = cache.clone()
    for b in range(1, B):
        want[:, b, :, pads[b]:pads[b] + C] = cache[:, 0, :, p0:p0 + C]
    return want
