"""The float64 reference of libindextts_score.so (include/indextts_score.h) on the kernel's OWN operands -- x rounded to the weight
type first for the 16-bit forms -- and the bounds the tests hold the device to.  Shared by
tests/test_score_*.py; nothing here calls the library.

Logit bound (the form of section 4.26):  E_l(r, j) = (D + 2) 2^-24 (sum_k |x W| + |b|): D products summed in fp32 (exact products in
the 16-bit forms) and one more addition for the bias.  E(r) = max_j E_l(r, j).
nll and lse:  2 E(r) + (V + 2) 2^-24 + EPS_FN -- every logit moves by at most E, so does the maximum the sum is taken relative to;
    V terms summed in fp32 and one log; EPS_FN is the error of the device's exp / log, which has no derivation here.  It was
    MEASURED as the rule says: the worst |lse_dev - lse_64| - (the other two terms) over the kernel test set on an MI355X, against
    this float64 reference (tests/test_score_kernels_gpu.py prints it per case), was EPS_FN_MEASURED = -2.3e-6 (fp32, D = 4,
    V = 1: the derived terms cover the device's exp / log on every row of every case); EPS_FN is EPS_FN_FACTOR = 4 times that,
    floored at 2^-20, hence the floor.  The largest |lse_dev - lse_64| outright was 6.2e-5 at D = 1280 (E = 4e-2) and 2.6e-3
    with the bias of 3e4 (E = 2.3).
rank:  |rank_dev - rank_64| <= the number of j != y with |l(j) - t| <= 2 E(r).
best:  the float64 argmax (smallest j) wherever every column within 2 E(r) of the maximum holds the maximum itself (exact copies).
Two float64 logits within TIE64 (1 + |l|) of each other count as EQUAL here: the float64 GEMM of the framework does not promise the
same summation order for two identical columns (it gave different last bits for copies in different tiles), while the device's two
logits of identical columns are the same bits by construction; TIE64 is four orders of magnitude under the smallest E of any case."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_small.npz")
EPS_FN_MEASURED = -2.3e-6        # worst excess over the two derived terms, see above (negative: they cover it)
EPS_FN_FACTOR = 4.0
TIE64 = 1e-9
EPS_FN = max(EPS_FN_FACTOR * EPS_FN_MEASURED, 2.0 ** -20)


def fixture():
    return np.load(FIXTURE)


def operands64(x, W, dtype):
    """(x, W) as the form of `dtype` multiplies them, in float64: x rounded once to the weight type."""
    return x.to(torch.float32).to(dtype).double(), W.double()


def reference(x, W, b, y, V, dtype, drop_bias=False, pad_columns=False, target_shift=0, reverse_ties=False, drop_range=None):
    """The quantities of the header in float64 from x fp32 [R, D], W [D, ldw] of `dtype`, b fp32 [V], y [R] (any integers).
    -> dict of t, lse, nll, rank, best, E [R], near [R] (the rank bound), decided [R] (the best check applies), logits [R, V].
    The keyword arguments are the NEGATIVE CONTROLS: each computes something the library must NOT compute."""
    xd, Wd = operands64(x, W, dtype)
    cols = W.shape[1] if pad_columns else V
    bd = torch.zeros(cols, dtype=torch.float64, device=x.device)
    if not drop_bias:
        bd[:V] = b.double()
    l = xd @ Wd[:, :cols] + bd
    if drop_range is not None:
        l[:, drop_range * 1024: (drop_range + 1) * 1024] = -float("inf")
    E = (x.shape[1] + 2) * 2.0 ** -24 * (xd.abs() @ Wd[:, :V].abs() + b.double().abs()).max(dim=1).values
    y = y.to(x.device).long()
    real = (y >= 0) & (y < V)
    ys = torch.where(real, (y + target_shift) % V, torch.zeros_like(y))
    t = l.gather(1, ys[:, None])[:, 0]
    lse = torch.logsumexp(l, dim=1)
    j = torch.arange(cols, device=x.device)[None]
    tie = (j > ys[:, None]) if reverse_ties else (j < ys[:, None])
    equal_t = (l - t[:, None]).abs() <= TIE64 * (1 + t[:, None].abs())
    rank = (((~equal_t & (l > t[:, None])) | (equal_t & tie)) & (j != ys[:, None])).sum(1)
    top = l.max(dim=1, keepdim=True).values
    at_top = l >= top - TIE64 * (1 + top.abs())
    best = at_top.to(torch.int64).argmax(dim=1) if not reverse_ties else cols - 1 - at_top.flip(1).to(torch.int64).argmax(dim=1)
    near = (((l - t[:, None]).abs() <= 2 * E[:, None]) & (j != ys[:, None])).sum(1)
    decided = ~((l >= top - 2 * E[:, None]) & ~at_top).any(dim=1)
    zero = torch.zeros_like(t)
    return dict(t=torch.where(real, t, zero), lse=lse, nll=torch.where(real, lse - t, zero), rank=torch.where(real, rank, torch.full_like(rank, -1)),
                best=best, E=E, near=torch.where(real, near, torch.zeros_like(near)), decided=decided, logits=l, real=real)


def float_bound(ref, V):
    """The bound on |nll_dev - nll_64| and |lse_dev - lse_64| per row."""
    return 2 * ref["E"] + (V + 2) * 2.0 ** -24 + EPS_FN


def mismatches(dev, ref, V):
    """The rows on which the device's outputs (dict of t, nll, lse, best, rank) miss the bounds against `ref`, as a dict
    name -> row indices (empty: all hold).  NaN on the device never passes."""
    fb = float_bound(ref, V)
    bad = {}

    def rows(mask):
        return mask.nonzero().reshape(-1).tolist()

    for k, bound in (("t", ref["E"]), ("lse", fb), ("nll", fb)):
        d = (dev[k].double() - ref[k]).abs()
        bad[k] = rows(~(d <= bound))
    bad["rank"] = rows((dev["rank"].long() - ref["rank"]).abs() > ref["near"])
    bad["rank_ignored"] = rows(~ref["real"] & (dev["rank"].long() != -1))
    bad["best"] = rows(ref["decided"] & (dev["best"].long() != ref["best"]))
    got = ref["logits"].gather(1, dev["best"].long().clamp(0, ref["logits"].shape[1] - 1)[:, None])[:, 0]
    bad["best_value"] = rows(~(got >= ref["logits"].max(dim=1).values - 2 * ref["E"]) | (dev["best"].long() < 0) | (dev["best"].long() >= V))
    return {k: v for k, v in bad.items() if v}
