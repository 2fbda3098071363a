"""Waveform finishing on the device, between the vocoder's fp32 samples (24 kHz, int16 range, as _vocode leaves them) and the PCM
encoder: trim leading and trailing silence, cap overlong pauses, set the level (libindextts_post.so, include/indextts_post.h,
DESIGN.md section 4.24).  24 kHz fp32 goes in and the same comes out, so it composes with every OutputFormat.

Two launches for any number of rows: ittp_frame_stats (sum of squares and peak of every 10 ms frame), a small device-to-host copy
(~100 frames per second of audio), the plan below, and ittp_splice (gather the kept pieces, fade them at the cuts, scale the row).
The plan is plain integer and float64 logic, so that the tests can hold it to their own restatement without a GPU.
"""
from __future__ import annotations

import math
import threading
from typing import NamedTuple

import numpy as np
import torch

from indextts import _native_post as natp

SRC_RATE = 24000
FRAME, FADE = natp.FRAME, natp.FADE
FULL_SCALE = 32768.0                       # 0 dBFS
MIN_KEEP_MS = FADE * 1000.0 / SRC_RATE     # 5 ms: the fade at a trimmed end lies inside the silence that is kept
MIN_PAUSE_MS = 2 * MIN_KEEP_MS             # 10 ms: each kept half of a capped pause holds one fade


def _number(name, v, lo, hi, none_ok=True):
    if v is None and none_ok:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not lo <= v <= hi:
        raise ValueError(f"PostProcess: {name} = {v!r} (a number in [{lo:g}, {hi:g}]{' or None' if none_ok else ''})")
    return float(v)


class PostProcess:
    """What to do to an utterance's samples; every step is off at None.
    trim_db        a 10 ms frame whose mean square lies below this level (dBFS, full scale 32768) is silent; leading and trailing
                   silence is cut down to keep_ms
    max_pause_ms   an inner run of silent frames longer than this is shortened to it: its first and last halves are kept and
                   joined with a 5 ms fade-out and fade-in (needs trim_db, which says what silence is)
    keep_ms        silence left at either end by the trim
    target_rms_db  the gain brings the RMS of the non-silent frames to this level ...
    peak_db        ... and is lowered, if needed, until no sample exceeds this one; -1 dBFS when a target is set and this is None.
                   Alone: peak normalisation."""
    __slots__ = ("trim_db", "max_pause_ms", "keep_ms", "target_rms_db", "peak_db")

    def __init__(self, trim_db=None, max_pause_ms=None, keep_ms=50, target_rms_db=None, peak_db=None):
        vals = (_number("trim_db", trim_db, -120.0, 0.0), _number("max_pause_ms", max_pause_ms, MIN_PAUSE_MS, 60000.0),
                _number("keep_ms", keep_ms, MIN_KEEP_MS, 60000.0, none_ok=False), _number("target_rms_db", target_rms_db, -60.0, 0.0),
                _number("peak_db", peak_db, -60.0, 0.0))
        if vals[1] is not None and vals[0] is None:
            raise ValueError("PostProcess: max_pause_ms needs trim_db (the level below which a frame is silent)")
        for k, v in zip(self.__slots__, vals):
            object.__setattr__(self, k, v)

    def __setattr__(self, *_):
        raise AttributeError("a PostProcess does not change")

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, PostProcess) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "PostProcess(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"

    @property
    def ceiling_db(self):
        """The peak ceiling in force: peak_db, -1 dBFS under a target without one, None without either."""
        return self.peak_db if self.peak_db is not None else -1.0 if self.target_rms_db is not None else None


class Plan(NamedTuple):
    pieces: tuple      # (src_off, dst_off, n, fade_in, fade_out) in output order: ittp_piece
    gain: float        # a value fp32 holds exactly
    n_out: int


def ramp_table() -> torch.Tensor:
    """The raised-cosine ramp of a cut, w[i] = (1 - cos(pi (i + 1/2) / FADE)) / 2: float64, rounded once to fp32.  A fade-in reads
    it forwards from the piece's first sample, a fade-out backwards from its last."""
    i = torch.arange(FADE, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(math.pi * (i + 0.5) / FADE)).to(torch.float32)


def _f32_at_most(v: float) -> float:
    """The largest fp32 value that does not exceed v."""
    f = np.float32(v)
    if float(f) > v:
        f = np.nextafter(f, np.float32(-np.inf))
    return float(f)


def plan(stats, n: int, pp: PostProcess) -> Plan:
    """The pieces, gain and output length of ONE row of n samples from its frame statistics [ceil(n / FRAME), 2]
    (sum of squares, peak per frame; ittp_frame_stats)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"post_wave.plan: a row of {n} samples has no frames (n >= 1)")
    st = np.asarray(stats, dtype=np.float64)
    F = -(-n // FRAME)
    if st.shape != (F, 2):
        raise ValueError(f"post_wave.plan: {n} samples are {F} frames: statistics [{F}, 2], not {list(st.shape)}")
    whole = Plan(((0, 0, n, 0, 0),), 1.0, n)
    count = np.full(F, float(FRAME))
    count[-1] = n - (F - 1) * FRAME                                       # the last frame holds the samples that exist
    floor = 0.0 if pp.trim_db is None else FULL_SCALE ** 2 * 10.0 ** (pp.trim_db / 10.0)
    loud = np.flatnonzero(~(st[:, 0] / count < floor))
    energy = float(st[loud, 0].sum())
    if loud.size == 0 or energy <= 0.0:
        return whole                                                      # nothing but silence: unchanged, gain 1
    first, last = int(loud[0]), int(loud[-1])
    lo, hi = 0, n
    if pp.trim_db is not None:
        keep = int(round(pp.keep_ms * SRC_RATE / 1000.0))
        lo, hi = max(0, first * FRAME - keep), min(n, (last + 1) * FRAME + keep)
    cuts = []                                                             # (where the kept head ends, where the kept tail starts)
    if pp.max_pause_ms is not None:
        room = int(round(pp.max_pause_ms * SRC_RATE / 1000.0))
        for a, b in zip(loud[:-1], loud[1:]):                             # the silent frames a + 1 .. b - 1 between two loud ones
            if (int(b) - int(a) - 1) * FRAME > room:
                cuts.append(((int(a) + 1) * FRAME + (room + 1) // 2, int(b) * FRAME - room // 2))
    pieces, src, dst, fade_in = [], lo, 0, FADE if lo > 0 else 0
    for head_end, tail_start in cuts:
        pieces.append((src, dst, head_end - src, fade_in, FADE))
        dst += head_end - src
        src, fade_in = tail_start, FADE
    pieces.append((src, dst, hi - src, fade_in, FADE if hi < n else 0))
    n_out = dst + hi - src
    gain = None
    if pp.target_rms_db is not None:
        rms = math.sqrt(energy / float(count[loud].sum()))
        gain = FULL_SCALE * 10.0 ** (pp.target_rms_db / 20.0) / rms
    if pp.ceiling_db is not None:
        peak = float(st[:, 1].max())
        ceiling = _f32_at_most(FULL_SCALE * 10.0 ** (pp.ceiling_db / 20.0))
        if peak > 0.0 and (gain is None or gain * peak > ceiling):
            gain = _f32_at_most(ceiling / peak)
            while gain * peak > ceiling:                                  # (exact in float64: both factors are fp32 values)
                gain = float(np.nextafter(np.float32(gain), np.float32(0.0)))
    gain = 1.0 if gain is None else _f32_at_most(gain)
    if not math.isfinite(gain) or gain > 3.0e38:
        raise ValueError(f"post_wave.plan: a gain of {gain!r} (non-silent RMS {math.sqrt(energy / float(count[loud].sum())):g})")
    return Plan(tuple(pieces), gain, n_out)


class PostWaveEngine:
    """process(waves, pp): ittp_frame_stats, the copy of the statistics, plan() per row, ittp_splice -- two launches for any
    number of rows.  Owns the fade ramp on `device` (written once) and nothing else that is shared: the sample, statistics,
    table and output tensors of a call are that call's own, so one engine may serve several threads and a result is never
    overwritten by a later call."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        natp.lib()
        self._ramp = ramp_table().to(self.device)
        self._lock = threading.Lock()
        self.launches = 0

    def _wave(self, w):
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != self.device:
            raise ValueError(f"PostWaveEngine: a waveform is an fp32 tensor on {self.device} (the vocoder's samples, int16 range)")
        return w.reshape(-1)

    def _pack(self, waves):
        """The rows in one buffer, each starting at a multiple of 4 elements (16 bytes): (x, [(x_off, n)])."""
        pad = torch.zeros(3, dtype=torch.float32, device=self.device)
        parts, rows, off = [], [], 0
        for w in waves:
            n = int(w.numel())
            rows.append((off, n))
            parts += [w, pad[: -n % 4]]
            off += n + (-n % 4)
        return torch.cat(parts), rows

    @torch.no_grad()
    def frame_stats(self, waves):
        """The frame statistics of fp32 device tensors [N_i >= 1]: a list of host arrays [ceil(N_i / FRAME), 2] (fp32)."""
        x, rows = self._pack([self._wave(w) for w in waves])
        return self._stats(x, rows)

    def _stats(self, x, rows):
        frames = [-(-n // FRAME) for _, n in rows]
        stats = torch.empty(len(rows), max(frames), 2, dtype=torch.float32, device=self.device)
        arr, raw = natp.table(natp.Row, rows)
        dev, (at,) = natp.upload(raw, device=self.device)
        natp.frame_stats(x, stats, arr, dev.data_ptr() + at)
        host = stats.cpu().numpy()                                        # (synchronises: the plan is host logic)
        return [host[r, :f] for r, f in enumerate(frames)]

    @torch.no_grad()
    def process(self, waves, pp: PostProcess, plans_out: list | None = None):
        """waves: fp32 device tensors [N_i] (whole utterances at 24 kHz).  Returns the list of their finished forms, fp32 device
        tensors [n_out_i]; each is bit-equal to that row processed alone.  A row without samples comes back as it is.
        plans_out, if given, receives the rows' plans (None for a row without samples)."""
        if not isinstance(pp, PostProcess):
            raise TypeError("PostWaveEngine.process: pp is a PostProcess")
        waves = [self._wave(w) for w in waves]
        live = [i for i, w in enumerate(waves) if w.numel()]
        outs, plans = list(waves), [None] * len(waves)
        if live:
            x, rows = self._pack([waves[i] for i in live])
            made = [plan(s, n, pp) for s, (_, n) in zip(self._stats(x, rows), rows)]
            out_rows, pieces, y_off = [], [], 0
            for (x_off, n), pl in zip(rows, made):
                out_rows.append((x_off, n, y_off, pl.n_out, len(pieces), len(pl.pieces), pl.gain, 0))
                pieces += pl.pieces
                y_off += (pl.n_out + 3) & ~3
            y = torch.empty(y_off, dtype=torch.float32, device=self.device)
            r_arr, r_raw = natp.table(natp.OutRow, out_rows)
            p_arr, p_raw = natp.table(natp.Piece, pieces)
            dev, (r_at, p_at) = natp.upload(r_raw, p_raw, device=self.device)
            natp.splice(x, y, self._ramp, r_arr, dev.data_ptr() + r_at, p_arr, dev.data_ptr() + p_at)
            with self._lock:
                self.launches += 2
            for i, r, pl in zip(live, out_rows, made):
                outs[i], plans[i] = y[r[2]: r[2] + r[3]], pl
        if plans_out is not None:
            plans_out[:] = plans
        return outs
