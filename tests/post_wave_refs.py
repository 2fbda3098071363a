"""A restatement in numpy float64 of waveform finishing (libindextts_post.so, indextts/utils/post_wave.py, DESIGN.md section
4.24): the two kernels and the host plan, written from the header's and the section's words alone -- it imports nothing from
indextts -- with the derived bounds and the inputs the tests share.

    frame f of a row of n samples covers [240 f, min(240 f + 240, n)):  ss = sum x^2,  pk = max |x|
    bound on ss:  (240 + 1) 2^-24 sum x^2 -- the worst case of a 240-term fp32 sum of fp32 squares in ANY order, with or without
                  fused multiply-adds (each term's rounding and each of at most 239 additions is one relative 2^-24)
    output j of a row, in piece (src, dst, n, fade_in, fade_out) at i = j - dst:  y = gain w x[src + i],
                  w = ramp[i] (i < fade_in), ramp[n - 1 - i] (n - 1 - i < fade_out), 1 elsewhere
    bound on y:   2 ulp of fp32 at |y| -- two multiplies, two roundings
"""
import math

import numpy as np

FRAME, FADE, RATE, FULL = 240, 120, 24000, 32768.0
U = 2.0 ** -24


def ramp32():
    """The raised-cosine ramp of a cut: float64, rounded once to fp32."""
    return np.array([0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / FADE) for i in range(FADE)], dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ frame stats
def frames(n):
    return (n + FRAME - 1) // FRAME


def frame_stats64(x, shift=0, partial_as_full=False, use_abs=True):
    """(ss [F], pk [F]) in float64 of fp32 samples x.  The controls: shift -- every frame starts `shift` samples late;
    partial_as_full -- the last frame's sum is taken for the mean over 240 samples times the samples that exist;
    use_abs=False -- the peak is the largest sample, not the largest magnitude."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    ss, pk = np.zeros(frames(n)), np.zeros(frames(n))
    for f in range(frames(n)):
        seg = x[f * FRAME + shift: min(n, (f + 1) * FRAME + shift)]
        if seg.size == 0:
            continue
        ss[f] = float(np.sum(seg * seg))
        if partial_as_full:
            ss[f] *= seg.size / FRAME
        pk[f] = float(np.max(np.abs(seg) if use_abs else seg))
    return ss, pk


def ss_bound(ss64):
    return (FRAME + 1) * U * ss64


# ----------------------------------------------------------------------------------------------------------------- splice
def splice64(x, pieces, gain, n_out):
    """The outputs in float64 over the fp32 ramp table; gain is taken as the fp32 value the launch carries."""
    x = np.asarray(x, dtype=np.float64)
    r = ramp32().astype(np.float64)
    g = float(np.float32(gain))
    y = np.full(n_out, np.nan)
    for src, dst, n, fi, fo in pieces:
        w = np.ones(n)
        w[:fi] = r[:fi]
        if fo:
            w[n - fo:] = r[:fo][::-1]
        y[dst:dst + n] = g * w * x[src:src + n]
    assert not np.isnan(y).any(), "the pieces do not cover the outputs"
    return y


def within_2ulp(got, want64):
    """|got - want| <= 2 ulp(fp32) at |want|, sample by sample (an exact zero must be a zero)."""
    got = np.asarray(got, dtype=np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return bool((np.abs(got - want64) <= 2.0 * ulp).all())


# ------------------------------------------------------------------------------------------------------------------- plan
def f32_down(v):
    f = np.float32(v)
    while float(f) > v:
        f = np.nextafter(f, np.float32(-np.inf))
    return float(f)


def frame_db(ss, cnt):
    ms = ss / cnt
    return -math.inf if ms <= 0.0 else 10.0 * math.log10(ms / FULL ** 2)


def plan64(ss, pk, n, trim_db=None, max_pause_ms=None, keep_ms=50, target_rms_db=None, peak_db=None):
    """(pieces, gain, n_out) of one row from its frame statistics, by the section's words:
    a frame is silent when its mean square in dBFS lies below trim_db; the silent runs at the ends are cut to keep_ms; an inner
    silent run longer than max_pause_ms keeps its first and last halves, joined by a fade-out and a fade-in; every cut end carries
    a fade; the gain takes the non-silent frames' RMS to target_rms_db and is lowered until gain x peak stays under the ceiling
    (peak_db, or -1 dBFS under a target); a row of silence alone is left as it is."""
    if n < 1:
        raise ValueError("no samples")
    F = frames(n)
    assert len(ss) == F and len(pk) == F
    cnt = [FRAME] * (F - 1) + [n - (F - 1) * FRAME]
    loud = [f for f in range(F) if not (trim_db is not None and frame_db(float(ss[f]), cnt[f]) < trim_db)]
    energy = sum(float(ss[f]) for f in loud)
    if not loud or energy <= 0.0:
        return [(0, 0, n, 0, 0)], 1.0, n
    start, stop = 0, n
    if trim_db is not None:
        keep = int(round(keep_ms * RATE / 1000.0))
        start = max(0, loud[0] * FRAME - keep)
        stop = min(n, (loud[-1] + 1) * FRAME + keep)
    spans = [[start, None]]                                   # kept source spans [from, to)
    if max_pause_ms is not None:
        room = int(round(max_pause_ms * RATE / 1000.0))
        for a, b in zip(loud, loud[1:]):
            run = (b - a - 1) * FRAME                         # samples of the silent frames between two loud ones
            if run > room:
                spans[-1][1] = (a + 1) * FRAME + (room - room // 2)
                spans.append([b * FRAME - room // 2, None])
    spans[-1][1] = stop
    pieces, dst = [], 0
    for k, (a, b) in enumerate(spans):
        fade_in = FADE if (k > 0 or start > 0) else 0
        fade_out = FADE if (k < len(spans) - 1 or stop < n) else 0
        pieces.append((a, dst, b - a, fade_in, fade_out))
        dst += b - a
    gain = 1.0
    if target_rms_db is not None:
        rms_db = 10.0 * math.log10(energy / sum(cnt[f] for f in loud) / FULL ** 2)
        gain = 10.0 ** ((target_rms_db - rms_db) / 20.0)
    ceiling_db = peak_db if peak_db is not None else (-1.0 if target_rms_db is not None else None)
    if ceiling_db is not None:
        peak = max(float(v) for v in pk)
        ceiling = f32_down(FULL * 10.0 ** (ceiling_db / 20.0))
        if peak > 0.0 and (target_rms_db is None or gain * peak > ceiling):
            gain = f32_down(ceiling / peak)
            while gain * peak > ceiling:
                gain = float(np.nextafter(np.float32(gain), np.float32(0.0)))
    return pieces, f32_down(gain), dst


# ----------------------------------------------------------------------------------------------------------------- inputs
def gauss(n, seed=0, amp=8000.0):
    return (np.random.default_rng(1000 + seed).standard_normal(n) * amp).astype(np.float32)


def db_amp(db):
    return FULL * 10.0 ** (db / 20.0)


def bursts(layout, seed=0, floor_db=None, burst_db=-12.0, tail=0):
    """A row for the engine tests: layout = [(kind, frames)], kind "s" a sine burst whose RMS is burst_db (440 Hz), "q" quiet:
    digital silence (floor_db None) or Gaussian noise whose RMS is floor_db; `tail` more quiet samples so that n is no multiple
    of 240.  fp32."""
    rng = np.random.default_rng(2000 + seed)
    parts, t = [], 0
    for kind, nf in layout + ([("q", 0)] if not tail else [("t", tail)]):
        m = nf * FRAME if kind != "t" else nf
        if kind == "s":
            parts.append(db_amp(burst_db) * math.sqrt(2.0) * np.sin(2 * math.pi * 440.0 * (t + np.arange(m)) / RATE + 0.3))
        elif floor_db is None:
            parts.append(np.zeros(m))
        else:
            parts.append(rng.standard_normal(m) * db_amp(floor_db))
        t += m
    return np.concatenate(parts).astype(np.float32)
