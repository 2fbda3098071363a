"""A float64 restatement of libindextts_codec.so (include/indextts_codec.h), on its own: the two launches,
the encoder chain, the bounds the GPU tests hold the kernels to, and the variants the negative controls need.  numpy only.

Bounds.  An fp32 sum of K products in ANY order, plus the bias and the residual, lies within (K + 2) 2^-24 (sum |w x| + |b| +
|resid|) of the exact value (each of the at most K + 2 roundings is relative 2^-24 of a partial sum that the sum of the
magnitudes bounds).  The same for a score: b(j) = (D + 2) 2^-24 (sum |z e_j| + h_j).  No measured number is in either."""
import os

import numpy as np

EPS = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "dvae_small.npz")
FRAMES = (1, 2, 3, 4, 5, 37, 160)
RELU_IN, RELU_OUT, RESIDUAL = 1, 2, 4


def out_rows(x_len, stride):
    return (x_len + stride - 1) // stride


def code_count(T):
    return ((T + 1) // 2 + 1) // 2


def conv(x, w, b, segs, stride, flags=0, resid=None, neighbour=False, phase=0, reverse_taps=False, drop_residual=False, swap_relu=False):
    """x [x_rows][Cin], w [Cout][Cin][taps] (the torch layout), b [Cout], segs of (x_row0, x_len, y_row0), resid [y_rows][Cout]:
    ({seg index: y float64 [y_len][Cout]}, {seg index: bound}).  The keyword variants are what a wrong kernel would compute:
    neighbour -- a row outside the clip read from the packed buffer (zero only outside the buffer); phase -- the input row of
    every tap moved by `phase`; reverse_taps; drop_residual; swap_relu -- the input ReLU applied to the output and the reverse."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    Cout, Cin, taps = w.shape
    pad = (taps - 1) // 2
    if swap_relu:
        flags = (flags & RESIDUAL) | (RELU_OUT if flags & RELU_IN else 0) | (RELU_IN if flags & RELU_OUT else 0)
    xin = np.maximum(x, 0.0) if flags & RELU_IN else x
    ys, bounds = {}, {}
    for s, (x0, n, y0) in enumerate(segs):
        m = out_rows(n, stride)
        acc = np.zeros((m, Cout))
        mag = np.zeros((m, Cout))
        t = np.arange(m)
        for tap in range(taps):
            i = t * stride + tap - pad + phase
            if neighbour:
                rows, ok = x0 + i, (x0 + i >= 0) & (x0 + i < x.shape[0])
            else:
                rows, ok = x0 + i, (i >= 0) & (i < n)
            g = np.where(ok[:, None], xin[np.clip(rows, 0, x.shape[0] - 1)], 0.0)
            wt = w[:, :, taps - 1 - tap if reverse_taps else tap].T                 # [Cin][Cout]
            acc += g @ wt
            mag += np.abs(g) @ np.abs(wt)
        acc += b
        mag += np.abs(b)
        if flags & RESIDUAL and not drop_residual:
            r = np.asarray(resid, dtype=np.float64)[y0: y0 + m]
            acc += r
            mag += np.abs(r)
        ys[s] = np.maximum(acc, 0.0) if flags & RELU_OUT else acc                   # (ReLU does not widen an error)
        bounds[s] = (taps * Cin + 2) * EPS * mag
    return ys, bounds


def within(got, want, bound):
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound))


def half_norms32(embed):
    """h[j] = |e_j|^2 / 2: float64, rounded once to fp32."""
    return (0.5 * (np.asarray(embed, dtype=np.float64) ** 2).sum(0)).astype(np.float32)


def scores(z, embed, h=None, omit_h=False):
    """(s64 [n][J], b [n][J]) of z [n][D] in embed [D][J] with the fp32 h the kernel is given (half_norms32 by default)."""
    z = np.asarray(z, dtype=np.float64)
    e = np.asarray(embed, dtype=np.float64)
    h = (half_norms32(embed) if h is None else np.asarray(h)).astype(np.float64)
    s = z @ e - (0.0 if omit_h else h)
    b = (z.shape[1] + 2) * EPS * (np.abs(z) @ np.abs(e) + h)
    return s, b


def choose(s, reverse_ties=False, skip_last=0):
    """argmax along the last axis, the smallest index among equals (the largest with reverse_ties); skip_last: the last
    `skip_last` codes are not looked at."""
    s = s[..., : s.shape[-1] - skip_last]
    if reverse_ties:
        return s.shape[-1] - 1 - np.argmax(s[..., ::-1], axis=-1)
    return np.argmax(s, axis=-1)


def audit(z, embed, codes, h=None):
    """The rows whose device code is NOT right: right is s64(code) >= max s64 - (b(code) + b(j*)); and where the margin to every
    other code exceeds 2 b the code EQUALS the float64 argmax.  Returns (list of bad rows, number of rows decided by margin)."""
    s, b = scores(z, embed, h)
    codes = np.asarray(codes)
    bad, decided = [], 0
    for r in range(s.shape[0]):
        c, j = int(codes[r]), int(np.argmax(s[r]))
        if not 0 <= c < s.shape[1] or s[r, c] < s[r, j] - (b[r, c] + b[r, j]):
            bad.append(r)
            continue
        others = np.delete(np.arange(s.shape[1]), j)
        if np.all(s[r, j] - s[r, others] > 2 * np.maximum(b[r, j], b[r, others])):
            decided += 1
            if c != j:
                bad.append(r)
    return bad, decided


# ----------------------------------------------------------------------------------------------------------- the fixture
def fixture():
    """tests/golden/dvae_small.npz as a dict: "sd" the state dict (numpy fp32), and per frame count T of FRAMES "mel" [100, T],
    "z32" and "z64" [T2, 32] from the reference class in fp32 and in .double(), "codes" [T2] from get_codebook_indices."""
    f = np.load(FIXTURE)
    out = {"sd": {k[3:]: f[k] for k in f.files if k.startswith("sd/")}}
    for T in FRAMES:
        out[T] = {name: f[f"{name}_{T}"] for name in ("mel", "z32", "z64", "codes")}
    return out


def plan(sd):
    """[(key, taps, stride, flags, starts a block)] of the encoder's convolutions in order."""
    n = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("encoder."))
    out = []
    for i in range(n):
        if f"encoder.{i}.0.weight" in sd:
            out.append((f"encoder.{i}.0", 3, 2, RELU_OUT, False))
        elif f"encoder.{i}.net.0.weight" in sd:
            out += [(f"encoder.{i}.net.0", 3, 1, RELU_OUT, True), (f"encoder.{i}.net.2", 3, 1, RELU_OUT, False),
                    (f"encoder.{i}.net.4", 1, 1, RESIDUAL, False)]
        else:
            out.append((f"encoder.{i}", 1, 1, 0, False))
    return out


def encoder64(sd, mel):
    """z [T2][D] in float64 of a mel [C][T]: the chain of conv() above on one clip."""
    x = np.asarray(mel, dtype=np.float64).T
    skip = None
    for key, taps, stride, flags, block in plan(sd):
        if block:
            skip = x
        ys, _ = conv(x, sd[key + ".weight"], sd[key + ".bias"], [(0, x.shape[0], 0)], stride, flags, skip if flags & RESIDUAL else None)
        x = ys[0]
    return x


def tau(fx):
    """The fixture's own max |z32 - z64|."""
    return max(float(np.max(np.abs(fx[T]["z32"].astype(np.float64) - fx[T]["z64"]))) for T in FRAMES)


def undecided(fx):
    """The frames of the fixture that are NOT decided, from the float64 z alone: a frame is decided when its margin
    s(best) - s(j) exceeds 4 tau |e_best - e_j|_1 (what a z within 4 tau of z64 can move the difference of two scores by) plus
    the search's rounding bound b(best) + b(j), for every j."""
    e = fx["sd"]["codebook.embed"].astype(np.float64)
    t4 = 4 * tau(fx)
    out = []
    for T in FRAMES:
        s, b = scores(fx[T]["z64"], fx["sd"]["codebook.embed"])
        for r in range(s.shape[0]):
            j = int(np.argmax(s[r]))
            need = t4 * np.abs(e[:, [j]] - e).sum(0) + b[r, j] + b[r]
            margin = s[r, j] - s[r]
            margin[j] = np.inf
            if not np.all(margin > need):
                out.append((T, r))
    return out
