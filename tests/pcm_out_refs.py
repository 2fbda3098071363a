"""References, bounds, stand-ins and negative controls of the PCM output back-end (libindextts_out.so).

Everything here is numpy on the host and written on its own, from the definitions -- feature_extractors.resample for the
polyphase sinc, ITU-T G.711 for the companders -- and shares no code with indextts/utils/pcm_out.py or csrc/pcmout.hip, so the
CPU tests can hold that module's tables to these, and the GPU tests the kernel.

Resample reference: float64 ON THE FP32-ROUNDED OPERANDS (samples, tap table), so the bound covers the kernel's arithmetic alone.
Bound, per output j (before the 2^-15 scaling of `f32`, which is exact):   (taps + 3) * 2^-24 * sum_t |kern[p][t]| * |x[.]|
    ONE fmaf chain over the taps: the classical bound of a recursive dot product of n terms with fused multiply-adds is
    gamma_n = n u / (1 - n u) times sum |a||b|, u = 2^-24; to first order taps * u, the three further units cover the second
    order (taps^2 u^2 < u for taps < 4000) with room.  The bound tests/melfront_refs.py uses for itta_resample.  Derived, not
    measured.

G.711, restated in integers the way the Recommendation's tables read: a segment SEARCH over the segment end points (the kernel
counts leading zeros instead).  mu-law: 14-bit magnitude from min(|s|, 32635) + 132, code = NOT(sign | segment << 4 | mantissa).
A-law: the 13-bit value s >> 3 (a negative one complemented), code = (segment << 4 | mantissa) XOR 0x55, sign bit set for s >= 0.
"""
import functools

import numpy as np

U = 2.0 ** -24
SRC = 24000
RATES = (8000, 16000, 48000, 44100, 22050, 11025, 24000)
ENCODINGS = ("f32", "pcm16", "mulaw", "alaw")
MU_CLIP, MU_BIAS = 32635, 132


def f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(acc, a, b):
    """fl32(acc + a * b) with one rounding: the product of two fp32 is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------------- plan
def plan(rate):
    """(orig, new, width, taps) of resample(., 24000, rate); the identity at 24 kHz is one tap of weight 1 (width 0)."""
    if rate == SRC:
        return 1, 1, 0, 1
    g = int(np.gcd(SRC, rate))
    orig, new = SRC // g, rate // g
    width = int(np.ceil(6 * orig / (0.99 * min(orig, new))))
    return orig, new, width, 2 * width + orig


def out_len(n, rate):
    orig, new, _, _ = plan(rate)
    return -(-new * n // orig)


@functools.lru_cache(maxsize=None)
def taps64(rate):
    """kern [new, taps] in float64, by the formula of feature_extractors.resample."""
    if rate == SRC:
        return np.ones((1, 1))
    orig, new, width, taps = plan(rate)
    base = min(orig, new) * 0.99
    idx = np.arange(-width, width + orig, dtype=np.float64)[None] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -6.0, 6.0)
    window = np.cos(t * np.pi / 6.0 / 2.0) ** 2
    t = t * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return sinc * window * (base / orig)


def taps32(rate):
    return f32(taps64(rate))


def _frames(x, rate, width_off=0):
    """[Q, taps]: frame q holds x[q orig + t - width], zeros outside [0, N).  width_off = 1 is the control `width off by one`:
    the same taps laid over the samples one position early."""
    orig, new, width, taps = plan(rate)
    width += width_off
    Q = -(-out_len(x.size, rate) // new)
    pad = np.zeros(width + Q * orig + taps, dtype=x.dtype)
    pad[width:width + x.size] = x
    return pad[np.arange(Q)[:, None] * orig + np.arange(taps)[None]]


def ref64(x32, rate, phase_shift=0, width_off=0):
    """(v64 [n_out], bound [n_out]) of fp32 samples x [N] in the int16 range: float64 over the fp32 table, and the derived worst
    case of the fp32 chain.  Both are in the units of `v`; the f32 encoding scales them by 2^-15.  phase_shift / width_off are
    the negative controls."""
    orig, new, width, taps = plan(rate)
    k = np.roll(taps32(rate), phase_shift, axis=0).astype(np.float64)
    fr = _frames(x32.astype(np.float64), rate, width_off)
    n = out_len(x32.size, rate)
    return (fr @ k.T).reshape(-1)[:n], (taps + 3) * U * (np.abs(fr) @ np.abs(k).T).reshape(-1)[:n]


def standin32(x32, rate, phase_shift=0, width_off=0):
    """The kernel's order of operations in fp32 on the host: one fmaf chain per output in ascending t."""
    orig, new, width, taps = plan(rate)
    k = np.roll(taps32(rate), phase_shift, axis=0)
    fr = _frames(x32, rate, width_off)
    acc = np.zeros((fr.shape[0], new), dtype=np.float32)
    for t in range(taps):
        acc = fma32(acc, fr[:, t:t + 1], k[None, :, t])
    return acc.reshape(-1)[:out_len(x32.size, rate)]


def excess(got32, v64, bound, scale=1.0):
    """max |got / scale - v64| / bound (0 / 0 counts as 0: an exact zero against a zero bound passes)."""
    err = np.abs(got32.astype(np.float64) / scale - v64)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


# --------------------------------------------------------------------------------------------------------------- encodings
def pcm16_of(v32, rounding="trunc"):
    """clamp to +-32767, then truncate toward zero: _vocode's clamp and numpy's astype (rounding="nearest" is a control)."""
    c = np.clip(v32.astype(np.float32), np.float32(-32767.0), np.float32(32767.0))
    return (np.rint(c) if rounding == "nearest" else np.trunc(c)).astype(np.int16)


MU_ENDS = np.array([0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF, 0x3FFF, 0x7FFF], dtype=np.int64)   # biased magnitude, per segment
A_ENDS = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF], dtype=np.int64)          # 13-bit magnitude, per segment


def mulaw_encode(s, bias=MU_BIAS):
    s = np.asarray(s).astype(np.int64)
    mag = np.minimum(np.abs(s), MU_CLIP) + bias
    seg = np.searchsorted(MU_ENDS, mag, side="left")                  # the first segment whose end is >= mag
    mant = (mag >> (seg + 3)) & 0xF
    return (~(np.where(s < 0, 0x80, 0) | (seg << 4) | mant) & 0xFF).astype(np.uint8)


def mulaw_decode(c):
    c = ~np.asarray(c).astype(np.int64) & 0xFF
    seg, mant = (c >> 4) & 7, c & 0xF
    mag = (((mant << 3) + MU_BIAS) << seg) - MU_BIAS
    return np.where(c & 0x80, -mag, mag).astype(np.int64)


def alaw_encode(s, xor=0x55):
    s = np.asarray(s).astype(np.int64)
    a = s >> 3                                                         # arithmetic: floor
    a = np.where(a >= 0, a, -a - 1)
    seg = np.searchsorted(A_ENDS, a, side="left")
    mant = np.where(seg < 2, a >> 1, a >> np.maximum(seg, 1)) & 0xF
    return ((((seg << 4) | mant) ^ xor) ^ np.where(s >= 0, 0x80, 0)).astype(np.uint8)


def alaw_decode(c):
    c = np.asarray(c).astype(np.int64) ^ 0x55
    seg, mant = (c >> 4) & 7, c & 0xF
    mag = np.where(seg == 0, (mant << 4) + 8, ((mant << 4) + 0x108) << np.maximum(seg - 1, 0))
    return np.where(c & 0x80, mag, -mag).astype(np.int64)


def encode(name, pcm16, **control):
    return {"mulaw": mulaw_encode, "alaw": alaw_encode}[name](pcm16, **control)


# ------------------------------------------------------------------------------------------------------------------ inputs
def lengths(rate):
    """N in {1, 2, width - 1, taps, 255, 256, 257, 1000, 4097}, those that are lengths."""
    _, _, width, taps = plan(rate)
    return sorted({n for n in (1, 2, width - 1, taps, 255, 256, 257, 1000, 4097) if n >= 1})


@functools.lru_cache(maxsize=None)
def gauss(n, seed=0):
    x = f32(np.random.default_rng(4230 + 7 * n + seed).normal(0.0, 8000.0, size=n))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def square(n=1000, period=37):
    """+-32767 (and beyond: every fifth half-wave at 1.5 x full scale, which only the clamp brings back)"""
    half = (np.arange(n) // period)
    x = f32(np.where(half % 2 == 0, 32767.0, -32767.0) * np.where(half % 5 == 4, 1.5, 1.0))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(rate, n, kind="gauss"):
    """(x32, v64, bound) of one row: computed once, shared, never written to."""
    x = gauss(n) if kind == "gauss" else square(n)
    v, b = ref64(x, rate)
    v.setflags(write=False)
    b.setflags(write=False)
    return x, v, b


def chunkings(n):
    """name -> the chunk lengths of an utterance of n samples: 256-aligned, ragged, and a stretch of 1-sample chunks."""
    def cut(sizes):
        out, left = [], n
        for s in sizes:
            s = min(s, left)
            out.append(s)
            left -= s
            if left == 0:
                return out
        return out + [left]
    return {"256-aligned": cut([256] * (n // 256)), "ragged": cut([1, 37, 300, 5, 0, 411, 2]),
            "one by one": cut([256, 100] + [1] * 48 + [3, 1, 1])}
