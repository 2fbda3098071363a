"""References, bounds, stand-ins and negative controls of the prompt audio front-end (libindextts_audio.so).

Everything here is numpy on the host and written on its own, from the definitions in feature_extractors.py (resample,
MelSpectrogramFeatures) -- it shares no code with indextts/utils/audio_engine.py, so the CPU tests can hold that module's tables
to these, and the GPU tests the kernels.

References are float64 ON THE FP32-ROUNDED OPERANDS (samples, tap table, bases, filterbank): the bound then covers the
kernel's arithmetic alone, not the rounding of its inputs.

Resample bound, per output j:   (taps + 3) * 2^-24 * sum_t |kern[p][t]| * |xbar[.]|
    The kernel forms xbar with C - 1 additions and one division (C <= 2 in every case here: at most 2 roundings, 2u relative,
    u = 2^-24) and runs ONE fmaf chain over the taps: the classical bound of a recursive dot product of n terms with fused
    multiply-adds is gamma_n = n u / (1 - n u) times sum |a||b| for ANY order.  To first order that is (taps + 2) u; the third
    unit covers the second-order terms ((taps + 2)^2 u^2 < u for taps < 4000).

Log-mel bound, per (mel m, frame t), in the LINEAR domain so that the clip floor cannot make it ill-conditioned:
    |exp(out) - max(mel64, 1e-7)| <= B + 2^-20 * max(mel64, 1e-7)
    B = sum_f fb[f, m] * (sqrt(2) * gamma * S_t + 2 * 2^-24 * mag64[t, f]) + (n_m + 1) * 2^-24 * mel64
    S_t = sum_n |x_n| w_n (every basis value is at most w_n in magnitude, so gamma S_t bounds the error of re and of im, and
    sqrt(2) gamma S_t that of the magnitude); gamma = (1024 + 2) * 2^-24: a 1024-term fmaf chain in any order, plus slack for the
    second order; 2 * 2^-24 mag: fl(sqrt(fma(re, re, fl(im im)))) is three roundings, 1 u after the square root plus its own;
    (n_m + 1) * 2^-24 mel: the n_m-term fmaf chain over the mel's bins; 2^-20: half an ulp of a log of magnitude < 16, plus logf's.
    A worst-case bound, derived, not measured.
"""
import functools

import numpy as np

U = 2.0 ** -24
N_FFT, HOP, N_BINS, N_MELS, SR = 1024, 256, 513, 100, 24000
GAMMA_TERMS = 1024
FLOOR = 1e-7

RATES = {"147->80": 44100, "2->1": 48000, "2->3": 16000, "147->160": 22050, "mean only": 24000}
MEL_LENGTHS = (513, 768, 4095, 4096, 4352)
MEL_SIGNALS = ("noise", "sine", "zeros", "impulse0", "impulseN")


def f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(acc, a, b):
    """fl32(acc + a * b) with one rounding: the product of two fp32 is exact in float64 (48 bits)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ inputs
def wave(C, N, seed):
    rng = np.random.default_rng(1000 + seed)
    return f32(rng.uniform(-1.0, 1.0, size=(C, N)))


def mel_signal(kind, N, seed=0):
    if kind == "noise":
        return f32(np.random.default_rng(77 + seed + N).uniform(-1.0, 1.0, size=N))
    if kind == "sine":          # bin 64 of 1024: 1500 Hz, on a bin centre -> most bins are at the floor
        return f32(0.5 * np.sin(2.0 * np.pi * 64.0 * np.arange(N) / N_FFT))
    x = np.zeros(N, dtype=np.float32)
    if kind == "impulse0":
        x[0] = 1.0
    elif kind == "impulseN":
        x[N - 1] = 1.0
    elif kind != "zeros":
        raise ValueError(kind)
    return x


# ---------------------------------------------------------------------------------------------------------------- resample
def resample_plan(sr):
    if sr == SR:
        return 1, 1, 0, 0
    g = int(np.gcd(sr, SR))
    orig, new = sr // g, SR // g
    width = int(np.ceil(6 * orig / (0.99 * min(orig, new))))
    return orig, new, width, 2 * width + orig


@functools.lru_cache(maxsize=None)
def taps64(sr):
    """kern [new, taps] in float64, by the formula of feature_extractors.resample."""
    orig, new, width, taps = resample_plan(sr)
    base = min(orig, new) * 0.99
    idx = np.arange(-width, width + orig, dtype=np.float64)[None] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -6.0, 6.0)
    window = np.cos(t * np.pi / 6.0 / 2.0) ** 2
    t = t * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return sinc * window * (base / orig)


def taps32(sr):
    return f32(taps64(sr))


def _tap_frames(xbar, sr, n_out):
    orig, new, width, taps = resample_plan(sr)
    Q = -(-n_out // new)
    pad = np.zeros(width + Q * orig + taps, dtype=xbar.dtype)
    pad[width:width + xbar.size] = xbar
    idx = np.arange(Q)[:, None] * orig + np.arange(taps)[None]
    return pad[idx]                                       # [Q, taps]: frame q holds xbar[q orig + t - width]


def resample_ref64(x32, sr, kern32=None):
    """(y64 [n_out], bound [n_out]) of planar fp32 x [C, N]: float64 on the fp32 operands."""
    C, N = x32.shape
    orig, new, width, taps = resample_plan(sr)
    xbar = x32.astype(np.float64).sum(0) / C
    if sr == SR:
        return xbar, 3 * U * np.abs(xbar)
    k = (taps32(sr) if kern32 is None else kern32).astype(np.float64)
    n_out = -(-new * N // orig)
    fr = _tap_frames(xbar, sr, n_out)
    y = (fr @ k.T).reshape(-1)[:n_out]
    bound = (taps + 3) * U * (np.abs(fr) @ np.abs(k).T).reshape(-1)[:n_out]
    return y, bound


def resample_standin32(x32, sr, kern32=None, phase_shift=0):
    """The kernel's order of operations in fp32: the channel mean in channel order, one fmaf chain in ascending t.
    phase_shift = 1 is the negative control `one phase's taps used for its neighbour`."""
    C, N = x32.shape
    orig, new, width, taps = resample_plan(sr)
    s = x32[0].copy()
    for c in range(1, C):
        s = (s + x32[c]).astype(np.float32)
    xbar = s if C == 1 else (s / np.float32(C)).astype(np.float32)
    if sr == SR:
        return xbar
    k = taps32(sr) if kern32 is None else kern32
    k = np.roll(k, phase_shift, axis=0)
    n_out = -(-new * N // orig)
    fr = _tap_frames(xbar, sr, n_out)
    acc = np.zeros((fr.shape[0], new), dtype=np.float32)
    for t in range(taps):
        acc = fma32(acc, fr[:, t:t + 1], k[None, :, t])
    return acc.reshape(-1)[:n_out]


# ----------------------------------------------------------------------------------------------------------------- log-mel
def hann64(kind="periodic"):
    n = np.arange(N_FFT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (N_FFT if kind == "periodic" else N_FFT - 1))


@functools.lru_cache(maxsize=None)
def bases32(window="periodic"):
    """(cos, sin) [1024, 513] with the window folded in, float64 rounded once to fp32."""
    k = np.arange(N_FFT, dtype=np.int64)[:, None]
    f = np.arange(N_BINS, dtype=np.int64)[None]
    ang = ((k * f) % N_FFT).astype(np.float64) * (2.0 * np.pi / N_FFT)
    w = hann64(window)[:, None]
    return f32(w * np.cos(ang)), f32(w * np.sin(ang))


@functools.lru_cache(maxsize=None)
def filterbank32():
    """mel_filterbank(513, 0, 12000, 100, 24000) as MelSpectrogramFeatures holds it: fp32 [513, 100]."""
    from indextts.utils.feature_extractors import mel_filterbank
    return mel_filterbank(N_BINS, 0.0, 12000.0, N_MELS, SR).numpy()


def mel_ranges(fb):
    rng = np.zeros((N_MELS, 2), dtype=np.int32)
    for m in range(N_MELS):
        nz = np.nonzero(fb[:, m])[0]
        if nz.size:
            rng[m] = nz[0], nz[-1] + 1
    return rng


def frames_of(x, hop=HOP, reflect="reflect"):
    """[T, 1024] with T = 1 + N // 256 whatever `hop` says (hop 255 is a negative control): centred, padded by 512."""
    N = x.size
    T = 1 + N // HOP
    p = np.pad(x, (N_FFT // 2, N_FFT // 2), mode=reflect)        # 'reflect': -i -> i; 'symmetric' repeats the edge (a control)
    idx = np.arange(T)[:, None] * hop + np.arange(N_FFT)[None]
    return p[idx]


def logmel_ref64(x32):
    """(mel64 [100, T] before clip and log, B [100, T]) from the fp32 samples, bases and filterbank, in float64."""
    c, s = bases32()
    fb = filterbank32().astype(np.float64)
    fr = frames_of(x32.astype(np.float64))
    mag = np.hypot(fr @ c.astype(np.float64), fr @ s.astype(np.float64))        # [T, 513]
    mel = mag @ fb                                                              # [T, 100]
    S = np.abs(fr) @ c[:, 0].astype(np.float64)                                 # the window is the cosine basis of bin 0
    gamma = (GAMMA_TERMS + 2) * U
    n_m = (fb > 0).sum(0)
    B = (np.sqrt(2.0) * gamma * S[:, None] * fb.sum(0)[None] + 2 * U * mel) + (n_m[None] + 1) * U * mel
    return mel.T.copy(), B.T.copy()


def mel_excess(out32, mel64, B):
    """max over every element of |exp(out) - max(mel64, 1e-7)| / (B + 2^-20 max(mel64, 1e-7)): <= 1 passes."""
    want = np.maximum(mel64, FLOOR)
    return float((np.abs(np.exp(out32.astype(np.float64)) - want) / (B + 2.0 ** -20 * want)).max())


KERNEL_K_ORDER = [16 * ks + 4 * g + j for ks in range(64) for j in range(4) for g in range(4)]


def logmel_standin32(x32, window="periodic", reflect="reflect", hop=HOP, fb_shift=0, clip_after_log=False):
    """The kernel's order of operations in fp32 (one fmaf chain per (frame, bin) over k in the order the MFMAs take it, the
    magnitude as sqrt(fma(re, re, im im)), one fmaf chain per mel over its bins in ascending order, clip, log); the keyword
    arguments are the negative controls."""
    c, s = bases32(window)
    fb = np.roll(filterbank32(), fb_shift, axis=0)
    fr = frames_of(x32, hop, reflect)
    re = np.zeros((fr.shape[0], N_BINS), dtype=np.float32)
    im = np.zeros_like(re)
    for k in KERNEL_K_ORDER:
        re = fma32(re, fr[:, k:k + 1], c[k][None])
        im = fma32(im, fr[:, k:k + 1], s[k][None])
    mag = np.sqrt(fma32((im * im).astype(np.float32), re, re).astype(np.float64)).astype(np.float32)
    rng = mel_ranges(fb)
    mel = np.zeros((fr.shape[0], N_MELS), dtype=np.float32)
    for m in range(N_MELS):
        for f in range(rng[m, 0], rng[m, 1]):
            mel[:, m] = fma32(mel[:, m], mag[:, f], np.full(fr.shape[0], fb[f, m], dtype=np.float32))
    with np.errstate(divide="ignore"):
        if clip_after_log:
            out = np.maximum(np.log(mel), np.float32(FLOOR))
        else:
            out = np.log(np.maximum(mel, np.float32(FLOOR)))
    return out.astype(np.float32).T.copy()


MEL_CONTROLS = {
    "symmetric Hann": dict(window="symmetric"),
    "reflection repeats the edge": dict(reflect="symmetric"),
    "hop 255": dict(hop=255),
    "mel triangles shifted one bin": dict(fb_shift=1),
    "clip after the log": dict(clip_after_log=True),
}


@functools.lru_cache(maxsize=None)
def mel_case(kind, N):
    """(x32, mel64, B) of one log-mel case: computed once, shared, never written to."""
    x = mel_signal(kind, N)
    mel, B = logmel_ref64(x)
    for a in (x, mel, B):
        a.setflags(write=False)
    return x, mel, B


def resample_cases():
    """(label, sr, C, N) of every single-wave resample case."""
    out = []
    for label, sr in RATES.items():
        orig = resample_plan(sr)[0]
        k = 7 if orig == 147 else 333 if orig == 2 else 777
        for C in (1, 2):
            for N in (orig * k, orig * k + 1, 1000):
                out.append((label, sr, C, N))
    return out


@functools.lru_cache(maxsize=None)
def resample_case(sr, C, N):
    x = wave(C, N, seed=sr % 97 + 10 * C + N)
    y, bound = resample_ref64(x, sr)
    for a in (x, y, bound):
        a.setflags(write=False)
    return x, y, bound


def resample_excess(got32, y64, bound):
    """max |got - y64| / bound (0 / 0 counts as 0: an exact zero against a zero bound passes)."""
    err = np.abs(got32.astype(np.float64) - y64)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())
