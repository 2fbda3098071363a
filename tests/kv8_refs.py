"""References of the FP8 KV cache tests (test_kv8_kernels_gpu.py): a paged E4M3 pool behind a ring block table built on the host,
its logical view, and float64 decode attention over decoded operands.  Nothing here calls the library under test; the quantiser
is indextts/utils/quant.py's host function, which test_kv8_cpu.py holds against torch's float8_e4m3fn cast."""
import math

import numpy as np
import torch

from indextts.utils import quant

TAB = 64           # ITTS_KV_TAB
P_FIRST = 256      # keys of itts_attn_decode_kv8's full pass (4 waves x 16 keys x 4 chunks); sized arms end at 64 / 128 / 192 / 256 slots
RPW = 16           # keys per wave-load: key groups are cut from pad & ~15


def rnd(*shape, seed=0, scale=1.0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(device)


def ring_table(spans, bs, seed):
    """spans: per row (lo, hi) positions, inclusive.  Every row gets the blocks of position indices lo // bs .. hi // bs at the ring
    slots (index % 64), block ids 1.. in shuffled order (0 = the scratch block).  Returns (table int32 [B][64], blocks)."""
    need = [hi // bs - lo // bs + 1 for lo, hi in spans]
    assert max(need) <= TAB - 2
    ids = np.random.default_rng(seed).permutation(np.arange(1, 1 + sum(need)))
    tab = np.zeros((len(spans), TAB), dtype=np.int32)
    o = 0
    for b, (lo, hi) in enumerate(spans):
        for bi in range(lo // bs, hi // bs + 1):
            tab[b, bi % TAB] = ids[o]
            o += 1
    return tab, 1 + sum(need)


def scatter(pool, tab, bs, b, positions, rows):
    """pool [blocks][H][bs][64] <- rows [H][n][64] at `positions` (list of ints) of table row b."""
    pos = np.asarray(positions, dtype=np.int64)
    blk = torch.from_numpy(tab[b, (pos // bs) % TAB].astype(np.int64)).to(pool.device)
    off = torch.from_numpy(pos % bs).to(pool.device)
    pool[blk, :, off] = rows.permute(1, 0, 2)


def gather(pool, tab, bs, b, positions):
    """[H][n][64] of `positions` of table row b."""
    pos = np.asarray(positions, dtype=np.int64)
    blk = torch.from_numpy(tab[b, (pos // bs) % TAB].astype(np.int64)).to(pool.device)
    off = torch.from_numpy(pos % bs).to(pool.device)
    return pool[blk, :, off].permute(1, 0, 2)


def attention(q, k, v, kn, vn, pads, pos, v_scale, lo_shift=0, new_key=True):
    """float64 softmax(q k / 8) v over the pool keys [pad_b + lo_shift, pos) of every row plus (new_key) the new key.
    q [B][H][64]; k, v [B][H][>= pos][64] DECODED AND K-SCALED keys, decoded values WITHOUT their scale; kn, vn [B][H][64] likewise;
    v_scale [H] multiplies the result.  Returns (ref, A) as [B][H * 64]; a row without any key gives NaN."""
    B, H, _ = q.shape
    dev = q.device
    s = torch.einsum("bhd,bhjd->bhj", q, k[:, :, :pos]) * 0.125
    j = torch.arange(pos, device=dev)[None, :]
    lo = torch.tensor(pads, device=dev)[:, None] + lo_shift
    s = s.masked_fill(~(j >= lo)[:, None, :], -math.inf)
    vv = v[:, :, :pos]
    if new_key:
        s = torch.cat([s, ((q * kn).sum(-1) * 0.125)[..., None]], -1)
        vv = torch.cat([vv, vn[:, :, None]], 2)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    p = p / p.sum(-1, keepdim=True)
    sc = v_scale.to(dev)[None, :, None]
    ref = torch.einsum("bhj,bhjd->bhd", p, vv) * sc
    A = torch.einsum("bhj,bhjd->bhd", p, vv.abs()) * sc
    return ref.reshape(B, H * 64), A.reshape(B, H * 64)


def decode_case(dtype, pads, pos, H, k_scale, v_scale, seed, device):
    """Operands of one launch with weight on the boundary keys: scores have a standard deviation of 2; the key at pad_b, the key
    in front of it, the first key of every 64-slot group and the NEW key are given a score near 6.
    Returns q, kn, vn (T, [B][H][64]: the step's query and new key / value), kc, vc (uint8 codes [B][H][pos + 1][64]: the logical
    cache, position pos holding stale codes the launch must overwrite)."""
    B = len(pads)
    q = (rnd(B, H, 64, seed=seed, device=device) * 2.0).to(dtype)
    qd = q.double()
    boost = 8.0 * 6.0 * qd / (qd * qd).sum(-1, keepdim=True)
    k = rnd(B, H, pos + 1, 64, seed=seed + 1, device=device)
    v = rnd(B, H, pos + 1, 64, seed=seed + 2, device=device)
    for b, p in enumerate(pads):
        b0 = p & ~(RPW - 1)
        for jm in {p, max(p - 1, 0)} | set(range(b0 + P_FIRST // 4, pos, P_FIRST // 4)):
            if jm <= pos:
                k[b, :, jm] = boost[b]
    kn = (boost * (1 + 0.01 * rnd(B, H, 64, seed=seed + 3, device=device))).to(dtype)
    vn = rnd(B, H, 64, seed=seed + 4, device=device).to(dtype)
    ks, vs = k_scale.to(device)[None, :, None, None], v_scale.to(device)[None, :, None, None]
    return q, kn, vn, quant.quantize_kv_e4m3(k, ks), quant.quantize_kv_e4m3(v, vs)
