"""What the token-selection kernels (csrc/sampling.hip, csrc/beam.hip) must DRAW, as distributions: the law of a token under the
Hugging Face warpers, the law of a beam-sample step, the Philox streams as the header documents them, and the statistics that hold
many draws to both.  Host only (numpy, float64).  This module imports neither tests/select_ref.py nor oracle/: select_ref restates
the kernels' rule operation by operation and is compared bit for bit; this is a second derivation, from the definitions, and is
compared statistically (tests/select_dist_sets.py builds the draw sets, tests/test_select_dist_{cpu,gpu}.py assert).

THE LAW (`law`), from the definitions of the transformers 4.44.2 processors in their call order:
  RepetitionPenaltyLogitsProcessor   score of every id that occurs in the history: s * penalty if s < 0 else s / penalty
  TemperatureLogitsWarper            s / temperature
  TopKLogitsWarper                   remove s < (k-th largest s)
  TopPLogitsWarper                   sort ascending, softmax, remove the ids whose cumulative probability is <= 1 - top_p, keep at
                                     least one
  softmax over what is left, one multinomial draw.
Ties at either boundary make the kept set depend on an order no definition gives; the draw sets keep their boundary gaps far above
select_ref's expf budget (asserted where the sets are built), and on such data the fp32 of the kernel moves a probability by ~1e-6
relative: three orders below what 65 536 draws resolve.

THE BEAM LAW (`beam_law`), step 0 of beam-sample (GenerationMixin._beam_search with do_sample): the scores of a beam are
log_softmax(logits) through the same processors (min_tokens_to_keep = 2 in top-p) plus the beam's running score; at step 0 every
beam but the first carries -1e9, so the pool is the first beam's kept candidates.  torch.multinomial(probs, 2 * num_beams) without
replacement is successive sampling: the first draw has probability p_a, the first two p_a p_b / (1 - p_a).  The drawn candidates
are then sorted by score (stable) and the best num_beams that are not the EOS go on.  `first` / `pair` are the laws of the draws in
draw order (observable on tied rows, where the stable sort keeps that order); `out_first` / `out_pair` are the laws of the tokens the
step emits for beams 0 and 1 (the two best of the 2 * num_beams drawn), by enumeration of the draw sequences.

STREAMS.  Philox4x32-10 (Salmon et al. 2011), first output word x0, u = (x0 >> 8) 2^-24.  Sampler counter (row | stream, step, 0, 0),
beam counter (batch element, step, draw, 0); key = seed + (state[5] << 32 | state[4]) mod 2^64.  `philox_x0` is vectorised over
numpy arrays; `SLIPS` are the ways a counter or key word can fail to reach it.

THE NIBBLE TRICK.  A row whose pool is 16 tokens of equal logit (top_k = 16, top_p = 1) turns the draw into floor(16 u): every
numerator is 1, every running sum an integer, `run > u * 16` exact in fp32.  Four bits of the draw are then read off the token, and
independence of two streams is a 16 x 16 contingency table.

STATISTICS.  Pearson chi-square against N p with bins merged (smallest expectation first) until each expects >= 5; the chi-square of
an r x c contingency table; the chi-square quantile from the regularised incomplete gamma function.  THE THRESHOLD IS A CONDITION:
every statistic lies below the 1 - 1e-9 quantile of its degrees of freedom.  All seeds are fixed, so nothing here is random at test
time; if a committed seed misses, the seed changes, never the quantile."""
import itertools
import math

import numpy as np

F64 = np.float64
M32 = 0xFFFFFFFF
ALPHA = 1e-9
SLIPS = ("row-dropped", "step-dropped", "seed-high-dropped", "carry-dropped", "draw-dropped")


# ------------------------------------------------------------------------------------------------------------------ the law
def warp(logits, history, settings, min_keep=1):
    """Scores after the four processors, float64 [V]; removed ids hold -inf.  settings: rep, temp, top_k, top_p."""
    s = np.array(logits, dtype=F64)
    V = s.shape[0]
    rep, temp, top_k, top_p = (float(settings[k]) for k in ("rep", "temp", "top_k", "top_p"))
    seen = sorted({int(i) for i in np.asarray(history).ravel() if 0 <= int(i) < V})
    if seen and rep != 1.0:
        s[seen] = np.where(s[seen] < 0, s[seen] * rep, s[seen] / rep)
    s = s / temp
    k = int(min(max(top_k, min_keep), V))
    kth = np.sort(s)[V - k]
    s[s < kth] = -np.inf
    if top_p < 1.0:
        order = np.argsort(s, kind="stable")                          # ascending
        z = s[order] - s.max()
        pr = np.exp(z) / np.exp(z).sum()
        remove = np.cumsum(pr) <= 1.0 - top_p
        remove[V - min_keep:] = False
        s[order[remove]] = -np.inf
    return s


def softmax(s):
    e = np.exp(s - s.max())
    return e / e.sum()


def law(logits, history, settings):
    """p[V]: the probability of each token."""
    return softmax(warp(logits, history, settings))


def wrong_law(logits, history, settings, what):
    """The law with one rule wrong: the negative controls.  Each is a proper distribution over the vocabulary."""
    st = dict(settings)
    if what == "temperature-ignored":
        st["temp"] = 1.0
    elif what == "penalty-ignored":
        st["rep"] = 1.0
    elif what == "penalty-wrong-side":                                # multiplied where it should divide and the reverse
        st["rep"] = 1.0 / settings["rep"]
    elif what in ("top_k+1", "top_k-1"):
        st["top_k"] = settings["top_k"] + (1 if what == "top_k+1" else -1)
    elif what in ("top_p-keep+1", "top_p-keep-1", "not-renormalised"):
        full = dict(settings, top_p=1.0)
        before = softmax(warp(logits, history, full))                 # the pool before the top-p cut
        kept = np.isfinite(warp(logits, history, settings))
        order = np.argsort(-before, kind="stable")
        n = int(kept.sum())
        if what == "not-renormalised":
            # `run > u * total` with the total of the uncut pool: the cut mass falls to the last kept token (the draw's fallback)
            p = np.where(kept, before, 0.0)
            p[order[n - 1]] += 1.0 - p.sum()
            return p
        n += 1 if what == "top_p-keep+1" else -1
        p = np.zeros_like(before)
        p[order[:n]] = before[order[:n]]
        return p / p.sum()
    else:
        raise KeyError(what)
    return law(logits, history, st)


def beam_law(logits, history, settings, num_beams, eos=-1):
    """Step 0 of beam-sample for one batch element whose first beam has `logits`.  Returns dict: p [V] (law of one draw from the full
    pool), first [V], pair [V, V] (first two draws, in draw order), out_first [V], out_pair [V, V] (tokens emitted for beams 0, 1)."""
    x = np.array(logits, dtype=F64)
    V = x.shape[0]
    logp = x - (x.max() + math.log(np.exp(x - x.max()).sum()))
    p = softmax(warp(logp, history, settings, min_keep=2))
    ids = np.nonzero(p > 0)[0]
    pair = np.zeros((V, V))
    for a in ids:
        for b in ids:
            if a != b:
                pair[a, b] = p[a] * p[b] / (1.0 - p[a])
    ndraw = min(2 * num_beams, ids.shape[0])
    out_pair = np.zeros((V, V))
    rank = {int(t): r for r, t in enumerate(sorted(ids, key=lambda t: (-p[t], t)))}
    for seq in itertools.permutations([int(t) for t in ids], ndraw):
        pr, rest = 1.0, 1.0
        for t in seq:
            pr *= p[t] / rest
            rest -= p[t]
        live = [t for t in sorted(seq, key=lambda t: rank[t]) if t != eos]   # (distinct scores: the sort is by score alone)
        out_pair[live[0], live[1]] += pr
    return dict(p=p, first=p, pair=pair, out_first=out_pair.sum(1), out_pair=out_pair)


# ------------------------------------------------------------------------------------------------------------------ streams
def philox_x0(c0, c1, c2, c3, k0, k1):
    """First output word of Philox4x32-10, vectorised: any mix of scalars and uint arrays that broadcast."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in (c0, c1, c2, c3, k0, k1)))
    m = np.uint64(M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0.astype(np.uint32)


def key_words(seed, s4, s5, slip=None):
    """(k0, k1) of the launch argument `seed` (64 bits) and the words state[4], state[5]."""
    seed, s4, s5 = int(seed) & (2 ** 64 - 1), int(s4) & M32, int(s5) & M32
    if slip == "seed-high-dropped":
        seed &= M32
    if slip == "carry-dropped":
        return ((seed & M32) + s4) & M32, ((seed >> 32) + s5) & M32
    k = (seed + ((s5 << 32) | s4)) & (2 ** 64 - 1)
    return k & M32, k >> 32


def sampler_u24(word0, step, seed, s45, slip=None):
    """x0 >> 8 (u = that times 2^-24) of the sampler's draws: word0 (row, or the record's stream) and step broadcast."""
    k0, k1 = key_words(seed, s45[0], s45[1], slip)
    word0, step = np.asarray(word0, dtype=np.uint64), np.asarray(step, dtype=np.uint64)
    if slip == "row-dropped":
        word0 = np.zeros_like(word0)
    if slip == "step-dropped":
        step = np.zeros_like(step)
    return philox_x0(word0, step, 0, 0, k0, k1) >> np.uint32(8)


def beam_u24(b, step, draw, seed, s45, slip=None):
    k0, k1 = key_words(seed, s45[0], s45[1], slip)
    draw = np.asarray(draw, dtype=np.uint64)
    if slip == "draw-dropped":
        draw = np.zeros_like(draw)
    return philox_x0(b, step, draw, 0, k0, k1) >> np.uint32(8)


def nibble(u24):
    """floor(16 u)."""
    return (np.asarray(u24) >> 20).astype(np.int64)


def without_replacement_ranks(u24_first, u24_second):
    """Two draws without replacement from 16 equal weights: (index of the first, rank of the second among the 15 left)."""
    a = nibble(u24_first)
    r = (np.asarray(u24_second).astype(np.int64) * 15) >> 24            # floor(15 u), exact in integers
    return a, r


# ------------------------------------------------------------------------------------------------------------------ statistics
def gammq(a, x):
    """Regularised upper incomplete gamma function Q(a, x) = Gamma(a, x) / Gamma(a): the series of P below a + 1, the continued
    fraction of Q (modified Lentz) above."""
    if x <= 0.0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(100000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return 1.0 - total * lead
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return lead * h


def chi2_sf(x, dof):
    return gammq(0.5 * dof, 0.5 * x)


def chi2_isf(q, dof):
    """The x with P(chi2_dof > x) = q (bisection on the monotone survival function, to 1e-10 relative)."""
    lo, hi = 0.0, float(dof) + 10.0
    while chi2_sf(hi, dof) > q:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if chi2_sf(mid, dof) > q:
            lo = mid
        else:
            hi = mid
        if hi - lo < 1e-10 * hi:
            break
    return 0.5 * (lo + hi)


_THRESHOLDS = {}


def threshold(dof):
    """The 1 - 1e-9 quantile of chi-square with `dof` degrees of freedom."""
    if dof not in _THRESHOLDS:
        _THRESHOLDS[dof] = chi2_isf(ALPHA, dof)
    return _THRESHOLDS[dof]


def chi2_gof(counts, p):
    """Pearson chi-square of `counts` against sum(counts) * p.  Bins are merged, smallest expectation first, until every bin
    expects >= 5 (a bin that expects 0 joins them: draws where the law has no mass are counted, not dropped).  Returns
    (statistic, degrees of freedom)."""
    counts, p = np.asarray(counts, dtype=F64).ravel(), np.asarray(p, dtype=F64).ravel()
    e = counts.sum() * p
    order = np.argsort(e, kind="stable")
    e, o = e[order], counts[order]
    bins_e, bins_o, acc_e, acc_o = [], [], 0.0, 0.0
    for ei, oi in zip(e, o):
        acc_e += ei
        acc_o += oi
        if acc_e >= 5.0:
            bins_e.append(acc_e)
            bins_o.append(acc_o)
            acc_e = acc_o = 0.0
    if acc_e > 0.0 or acc_o > 0.0:                                     # the remainder joins the smallest finished bin
        if bins_e:
            bins_e[0] += acc_e
            bins_o[0] += acc_o
        else:
            bins_e.append(acc_e)
            bins_o.append(acc_o)
    be, bo = np.array(bins_e), np.array(bins_o)
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = float(np.where(be > 0, (bo - be) ** 2 / be, np.where(bo > 0, np.inf, 0.0)).sum())
    return stat, max(len(bins_e) - 1, 1)


def chi2_table(a, b, na=16, nb=16):
    """Chi-square of independence of the na x nb contingency table of the paired samples a (0 .. na - 1) and b (0 .. nb - 1).
    Returns (statistic, (na - 1)(nb - 1)).  Every row and column has to occur: a margin of zero is a failure of its own."""
    a, b = np.asarray(a, dtype=np.int64).ravel(), np.asarray(b, dtype=np.int64).ravel()
    t = np.bincount(a * nb + b, minlength=na * nb).reshape(na, nb).astype(F64)
    e = np.outer(t.sum(1), t.sum(0)) / t.sum()
    if (e == 0).any():
        return math.inf, (na - 1) * (nb - 1)
    return float(((t - e) ** 2 / e).sum()), (na - 1) * (nb - 1)
