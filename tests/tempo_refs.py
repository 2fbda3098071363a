"""A restatement in numpy float64 of the speaking rate (libindextts_tempo.so, indextts/utils/tempo.py):
WSOLA as include/indextts_tempo.h states it, written from the header's words alone -- it imports nothing from indextts -- with the
derived bounds, the decision audit, the negative controls and the inputs the tests share.

    xz[i] = x[i] inside [0, n), 0 outside;  S = round(1024 speed)
    n_out = max(1, (1024 n + S // 2) // S),  K = (n_out - 1) // HOP + 2,  a_k = (k HOP S + 512) // 1024 - HOP
    p_0 = -HOP, d_0 = 0;  t[i] = xz[p_(k-1) + HOP + i];  c(d) = sum_(i < WIN) t[i] xz[a_k + d + i], -TOL <= d < TOL
    d_k = argmax c; of equal scores the smallest |d|, of +-d the negative one;  p_k = a_k + d_k
    y[m] = w[HOP + j] xz[p_k0 + HOP + j] + w[j] xz[p_(k0+1) + j],  j = m mod HOP, k0 = m // HOP

    bound on c:  b(d) = (WIN + 1) 2^-24 sum |t[i] xz[a_k + d + i]| -- the worst case of an fp32 sum of WIN rounded products in ANY
                 order, with or without fused multiply-adds (each term's rounding and each of at most WIN - 1 additions is one
                 relative 2^-24, to first order; the + 1 covers the second)
    the audit:   discrete choices are not compared through the chain -- one near-tie would change everything after it.  Given the
                 device's OWN d_(k-1), frame k is right when c64(d_dev) >= max_d c64(d) - (b(d_dev) + b(d*)): no lag beats the
                 chosen one by more than the two sums' errors.  A frame whose products are all exactly zero has every fp32 score
                 exactly zero: the tie rule decides, d = 0.
    bound on y:  3 2^-24 (|w x|_1 + |w x|_2): two products and one sum, three roundings at most (a fused multiply-add saves one)
"""
import math

import numpy as np

HOP, WIN, TOL, RATE = 384, 768, 192, 24000
ONE, S_MIN, S_MAX = 1024, 512, 2048
U = 2.0 ** -24
LAGS = np.arange(-TOL, TOL)


def fixed_speed(speed):
    return int(math.floor(speed * ONE + 0.5))


def out_len(n, S):
    return max(1, (n * ONE + S // 2) // S)


def frames(n, S):
    return (out_len(n, S) - 1) // HOP + 2


def nominal(k, S):
    return (k * HOP * S + 512) // ONE - HOP


def window32():
    """The Hann window: float64, rounded once to fp32."""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / WIN) for i in range(WIN)], dtype=np.float64).astype(np.float32)


def xz(x, start, length):
    """xz[start : start + length] in float64."""
    n = x.size
    out = np.zeros(length)
    lo, hi = max(start, 0), min(start + length, n)
    if hi > lo:
        out[lo - start: hi - start] = x[lo:hi]
    return out


def scores(x, S, k, p_prev, template_at=HOP):
    """(c [2 TOL], b [2 TOL]) of frame k >= 1 in float64, entry TOL + d for the lag d, given p_(k-1).  template_at is where the
    template starts past p_(k-1): HOP (anything else is a control)."""
    t = xz(x, p_prev + template_at, WIN)
    span = xz(x, nominal(k, S) - TOL, WIN + 2 * TOL)
    c = np.correlate(span, t, "valid")[: 2 * TOL]
    b = (WIN + 1) * U * np.correlate(np.abs(span), np.abs(t), "valid")[: 2 * TOL]
    return c, b


def choose(c, reverse_ties=False):
    """The lag of largest c; of equal scores the smallest |d|, of +-d the negative one (reverse_ties, a control: the largest |d|,
    the positive one)."""
    tied = LAGS[c == c.max()]
    key = np.abs(tied) * 2 + (tied > 0)
    return int(tied[np.argmax(key) if reverse_ties else np.argmin(key)])


class Frame:
    __slots__ = ("k", "d", "silent", "ambiguous", "margin", "b")


def chain(x, S):
    """The reference's own chain: [Frame] for k = 1 .. K - 1 (d_0 = 0 is not listed).
    silent: every product of every lag is exactly zero.  ambiguous: some other lag lies within 2 b of the best (b the larger of
    the two lags' bounds) -- but two lags whose products are ALL exactly zero are not ambiguous: their fp32 scores are exactly
    zero too, and the tie rule decides between them on the device as it does here.
    margin: how far the nearest other lag lies below the best; b: the best lag's bound."""
    x = np.asarray(x, dtype=np.float64)
    out, p = [], -HOP
    for k in range(1, frames(x.size, S)):
        c, b = scores(x, S, k, p)
        f = Frame()
        f.k, f.d = k, choose(c)
        best = f.d + TOL
        f.silent = bool((b == 0.0).all())
        gap = c[best] - c
        near = (gap <= 2.0 * np.maximum(b, b[best])) & ~((b == 0.0) & (b[best] == 0.0))
        near[best] = False
        f.ambiguous = bool(near.any())
        f.margin = float(np.delete(gap, best).min())
        f.b = float(b[best])
        out.append(f)
        p = nominal(k, S) + f.d
    return out


def audit(x, S, offsets, template_at=HOP):
    """The frames at which the lags `offsets` [K] (the device's) are wrong, each judged given the lag before it: [(k, why)]."""
    x = np.asarray(x, dtype=np.float64)
    K = frames(x.size, S)
    off = [int(v) for v in offsets]
    bad = []
    if len(off) != K:
        return [(-1, f"{len(off)} lags for K = {K}")]
    if off[0] != 0:
        bad.append((0, "d_0 is not 0"))
    p = -HOP + off[0]
    for k in range(1, K):
        d = off[k]
        if not -TOL <= d < TOL:
            bad.append((k, f"the lag {d} is outside [-TOL, TOL)"))
            d = max(-TOL, min(TOL - 1, d))
        c, b = scores(x, S, k, p, template_at)
        star = choose(c)
        if (b == 0.0).all():
            if d != 0:
                bad.append((k, f"a silent frame at the lag {d}"))
        elif c[d + TOL] < c[star + TOL] - (b[d + TOL] + b[star + TOL]):
            bad.append((k, f"the lag {d} scores {c[d + TOL]:.9g}, the lag {star} {c[star + TOL]:.9g}: more than the bound "
                           f"{b[d + TOL] + b[star + TOL]:.3g} apart"))
        p = nominal(k, S) + d
    return bad


def overlap_add(x, S, offsets, swap_halves=False, p_shift=0):
    """(y [n_out], bound [n_out]) in float64 over the fp32 window, with the lags `offsets`.  The controls: swap_halves -- the
    rising half weights the falling piece and the other way round; p_shift -- every p_k taken that much too late."""
    x = np.asarray(x, dtype=np.float64)
    w = window32().astype(np.float64)
    n_out = out_len(x.size, S)
    wa, wb = (w[:HOP], w[HOP:]) if swap_halves else (w[HOP:], w[:HOP])
    y, bound = np.zeros(n_out), np.zeros(n_out)
    for k0 in range((n_out - 1) // HOP + 1):
        m0 = k0 * HOP
        cnt = min(HOP, n_out - m0)
        pa = nominal(k0, S) + int(offsets[k0]) + p_shift
        pb = nominal(k0 + 1, S) + int(offsets[k0 + 1]) + p_shift
        one = wa[:cnt] * xz(x, pa + HOP, cnt)
        two = wb[:cnt] * xz(x, pb, cnt)
        y[m0: m0 + cnt] = one + two
        bound[m0: m0 + cnt] = 3.0 * U * (np.abs(one) + np.abs(two))
    return y, bound


def within(got, want, bound):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - want) <= bound).all())


# ------------------------------------------------------------------------------------------------------------------ inputs
def speechlike(n, seed):
    """fp32 [n], int16 range: twelve harmonics on an f0 that glides between 90 and 250 Hz, under a syllable-like envelope, plus
    faint noise; from 6000 samples on, two gaps of n / 10 exact zeros (at 0.3 n and 0.7 n).  Not a stationary tone: the lags one
    period apart do not tie."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = 170.0 + 80.0 * np.sin(2.0 * math.pi * rng.uniform(0.9, 1.6) * t + rng.uniform(0, 2 * math.pi))
    phase = 2.0 * math.pi * np.cumsum(f0) / RATE
    sig = np.zeros(n)
    for h in range(1, 13):
        sig += rng.uniform(0.5, 1.0) / h ** 1.2 * np.sin(h * phase + rng.uniform(0, 2 * math.pi))
    env = 0.55 + 0.45 * np.sin(2.0 * math.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 2 * math.pi))
    x = 9000.0 * env * sig / max(1e-9, np.abs(sig).max()) + 3.0 * rng.standard_normal(n)
    if n >= 6000:
        for at in (0.3, 0.7):
            x[int(at * n): int(at * n) + n // 10] = 0.0
    return x.astype(np.float32)


def tone(n, hz=200.0, amp=8000.0):
    return (amp * np.sin(2.0 * math.pi * hz * np.arange(n) / RATE)).astype(np.float32)


# the rows of the kernel tests: (n, S, seed) -- every n of {1, 383, 384, 385, 769, 2400, 24000}, every S of {512, 819, 1024, 1280,
# 2048}, both ends of the speed range at short and at long rows
CASES = ((1, 512, 1), (1, 1024, 2), (1, 2048, 3), (383, 2048, 4), (384, 512, 5), (385, 819, 6), (769, 1280, 7), (769, 512, 8),
         (2400, 2048, 9), (2400, 819, 10), (24000, 512, 11), (24000, 819, 12), (24000, 1024, 13), (24000, 1280, 14), (24000, 2048, 15))


def case_rows():
    return [speechlike(n, seed) for n, _, seed in CASES]
