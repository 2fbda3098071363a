"""The speaking rate on the device, between the vocoder's fp32 samples (24 kHz, int16 range, as _vocode leaves them) and waveform
finishing: WSOLA time-scale modification (libindextts_tempo.so, include/indextts_tempo.h).  24 kHz fp32
goes in and the same comes out, shorter or longer, at the same pitch; so it composes with post= and with every OutputFormat.

Two launches for any number of rows: ittm_search (the chain of lags of every row, one workgroup per row) and ittm_overlap_add.
The lengths are plain integer arithmetic, so that the tests can hold them to their own restatement without a GPU.

Pitch is the classical two-step shift on top of it: for p = 2^(semitones / 12) and a speed s, WSOLA at the
rate s / p (the duration becomes p / s, the pitch stays), then resampling by p (libindextts_pitch.so, include/indextts_pitch.h:
output m reads the input at m p), which brings the duration to 1 / s and multiplies every frequency by p.  The formants move with
the pitch, as with any resampling shifter: a voice shifted far up sounds smaller, far down larger.  One more launch for any number
of rows; pitch_plan() and resample_ratio_ref() state its integers and its sums without a GPU.
"""
from __future__ import annotations

import math
import threading

import numpy as np
import torch

from indextts import _native_pitch as natr
from indextts import _native_tempo as natm

HOP, WIN, TOL = natm.HOP, natm.WIN, natm.TOL
SPEED_ONE, SPEED_MIN, SPEED_MAX = natm.SPEED_ONE, natm.SPEED_MIN, natm.SPEED_MAX


def fixed_speed(speed) -> int:
    """S = round(1024 speed) of a speed in [0.5, 2.0] (a half rounds up).  Anything else -- a bool, a string, a value that is not
    finite or out of range -- is a ValueError."""
    if isinstance(speed, bool) or not isinstance(speed, (int, float, np.integer, np.floating)) or not math.isfinite(speed) \
            or not 0.5 <= speed <= 2.0:
        raise ValueError(f"speed = {speed!r} (a number in [0.5, 2.0]: 0.8 is a fifth slower, 1.25 a quarter faster)")
    return int(math.floor(float(speed) * SPEED_ONE + 0.5))


def _fixed(S) -> int:
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not SPEED_MIN <= S <= SPEED_MAX:
        raise ValueError(f"S = {S!r} (an integer in [{SPEED_MIN}, {SPEED_MAX}]: fixed_speed(speed))")
    return int(S)


def out_len(n: int, S: int) -> int:
    """The outputs of a row of n >= 1 samples at the speed S / 1024."""
    n, S = int(n), _fixed(S)
    if n < 1:
        raise ValueError(f"tempo.out_len: a row of {n} samples (n >= 1)")
    return max(1, (n * SPEED_ONE + S // 2) // S)


def frames(n: int, S: int) -> int:
    """K: the frames, and lags, of a row of n >= 1 samples at the speed S / 1024."""
    return (out_len(n, S) - 1) // HOP + 2


def window_table() -> torch.Tensor:
    """The Hann window w[i] = 1/2 - 1/2 cos(2 pi i / WIN): float64, rounded once to fp32.  Its halves HOP apart sum to one."""
    i = torch.arange(WIN, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * i / WIN)).to(torch.float32)


# ------------------------------------------------------------------------------------------------------------------- pitch
PITCH_MAX = 12.0                                    # semitones either way: p in [1/2, 2]
STEP_ONE = 1 << 32                                  # p = 1 in 32.32 fixed point


def pitch_plan(semitones, speed=None):
    """(wsola_rate, step, out_len) of a shift by `semitones` at the speed `speed` (None: 1): WSOLA runs at wsola_rate = speed / p
    (S = fixed_speed(wsola_rate)), the resampler at step = round(p 2^32), and out_len(n_in) = ceil(n_in 2^32 / step) is the
    number of outputs it gives for n_in samples -- the most that read no position past the last sample.  -12 <= semitones <= 12,
    and speed / p must be a rate WSOLA takes (0.5 .. 2.0); anything else is a ValueError that names both numbers."""
    s = 1.0 if speed is None else speed
    fixed_speed(s)
    if isinstance(semitones, bool) or not isinstance(semitones, (int, float, np.integer, np.floating)) or not math.isfinite(semitones) \
            or not -PITCH_MAX <= semitones <= PITCH_MAX:
        raise ValueError(f"pitch = {semitones!r} (semitones, a number in [-12, 12]: 12 is an octave up) at speed = {s!r}")
    p = 2.0 ** (float(semitones) / 12.0)
    rate = float(s) / p
    if not 0.5 <= rate <= 2.0:
        raise ValueError(f"pitch = {semitones!r} semitones at speed = {s!r}: the time stretch would run at speed / 2^(pitch / 12) = "
                         f"{rate:.4f}, outside [0.5, 2.0]")
    step = int(round(p * STEP_ONE))

    def resampled_len(n_in: int) -> int:
        return -((-int(n_in) * STEP_ONE) // step)

    return rate, step, resampled_len


def cutoff_of(step: int) -> int:
    """The filter's scale c = min(1, 1 / p) in units of 2^-16, rounded to nearest: the cutoff of a downsampling row lies at the
    Nyquist frequency of its output."""
    return min(natr.CUTOFF_ONE, ((1 << 48) + step // 2) // step)


def ratio_table() -> torch.Tensor:
    """G of include/indextts_pitch.h: h(u) = sinc(u) cos^2(pi u / (2 HW)) at u = k / PHASES - HW -- the Hann-windowed sinc of
    half-width 6 that feature_extractors.resample and pcm_out use, without their roll-off, so that it is 1 at 0 and 0 at the
    other integers (set exactly) -- float64, rounded once to fp32, closed by zeros."""
    k = torch.arange(natr.TABLE, dtype=torch.float64)
    u = k / natr.PHASES - natr.HW
    t = u * math.pi
    h = torch.where(u == 0, torch.ones_like(u), torch.sin(t) / t) * torch.cos(t / (2 * natr.HW)) ** 2
    whole = (torch.arange(natr.TABLE) % natr.PHASES) == 0
    h[whole] = 0.0
    h[natr.HW * natr.PHASES] = 1.0
    h[2 * natr.HW * natr.PHASES:] = 0.0
    return h.to(torch.float32)


def resample_ratio_ref(x, step: int, n_out: int | None = None, cutoff: int | None = None, table=None, detail: bool = False):
    """The float64 statement of ittr_resample_ratio for one row x (include/indextts_pitch.h): the same integers, the same fp32
    table, the weights and the sum in float64.  n_out None: ceil(n 2^32 / step); cutoff None: cutoff_of(step).  detail: also the
    sum of |w_j xz[i]| cutoff 2^-16 per output, what an error bound of the fp32 sum is stated in."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n, step = int(x.size), int(step)
    cutoff = cutoff_of(step) if cutoff is None else int(cutoff)
    if n < 1 or not natr.STEP_MIN <= step <= natr.STEP_MAX or not natr.CUTOFF_MIN <= cutoff <= natr.CUTOFF_ONE:
        raise ValueError(f"resample_ratio_ref: n = {n}, step = {step}, cutoff = {cutoff}")
    n_out = -((-n * STEP_ONE) // step) if n_out is None else int(n_out)
    table = ratio_table() if table is None else table
    G = np.asarray(table.cpu().numpy() if torch.is_tensor(table) else table, dtype=np.float64)
    HW = natr.HW
    H = (HW * natr.CUTOFF_ONE + cutoff - 1) // cutoff
    pos = np.arange(n_out, dtype=np.int64) * np.int64(step)
    i0, f = pos >> 32, pos & np.int64(0xffffffff)
    U = (((f + (np.int64(H - 1) << 32)) * np.int64(cutoff)) >> 16) + (np.int64(HW) << 32)
    y, mass = np.zeros(n_out), np.zeros(n_out)
    for j in range(2 * H):
        i = i0 - H + 1 + j
        Uj = U - j * (cutoff << 16)
        inside = (Uj >= 0) & (Uj < (2 * HW) << 32)
        k = np.where(inside, Uj >> 24, 0)
        t = (Uj & 0xffffff).astype(np.float64) * 2.0 ** -24
        w = np.where(inside, G[k] + t * (G[k + 1] - G[k]), 0.0)
        term = w * np.where((i >= 0) & (i < n), x[np.clip(i, 0, n - 1)], 0.0)
        y += term
        mass += np.abs(term)
    gain = cutoff / natr.CUTOFF_ONE
    return (y * gain, mass * gain) if detail else y * gain


class TempoEngine:
    """process(wavs, speeds): ittm_search and ittm_overlap_add -- two launches for any number of rows.  Owns the window on
    `device` (written once) and nothing else that is shared: the sample, lag, table and output tensors of a call are that call's
    own, so one engine may serve several threads and a result is never overwritten by a later call.
    resample(wavs, steps): ittr_resample_ratio, one launch more; shift(rows, lengths, pitch, speed): process at speed / p, then
    resample by p -- the pitch shift.  The resampler's table is written at the first shift and kept."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        natm.lib()
        self._window = window_table().to(self.device)
        self._taps = None                                    # the resampler's table: uploaded at the first shift, then kept
        self._lock = threading.Lock()
        self.launches = 0

    def _wave(self, w):
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != self.device:
            raise ValueError(f"TempoEngine: a waveform is an fp32 tensor on {self.device} (the vocoder's samples)")
        return w

    @torch.no_grad()
    def process(self, wavs, speeds, offsets_out: list | None = None):
        """wavs: fp32 device tensors [N_i] (whole utterances at 24 kHz); speeds: one per row -- None, or S = fixed_speed(speed).
        Returns the list of their forms at those speeds, fp32 device tensors [out_len(N_i, S_i)], each bit-equal to that row
        processed alone.  A row at None or at S = 1024, and a row without samples, comes back as the same tensor object.
        offsets_out, if given, receives the rows' lags (int32 device tensors [frames(N_i, S_i)]; None for a row passed through)."""
        wavs = [self._wave(w) for w in wavs]
        if len(speeds) != len(wavs):
            raise ValueError(f"TempoEngine.process: {len(speeds)} speeds for {len(wavs)} rows")
        speeds = [None if s is None else _fixed(s) for s in speeds]
        live = [i for i, (w, s) in enumerate(zip(wavs, speeds)) if s is not None and s != SPEED_ONE and w.numel()]
        outs, lags = list(wavs), [None] * len(wavs)
        if live:
            pad = torch.zeros(3, dtype=torch.float32, device=self.device)
            parts, rows, x_off, o_off, y_off = [], [], 0, 0, 0
            for i in live:                                   # every row starts at a multiple of 4 elements (16 bytes)
                n, S = int(wavs[i].numel()), speeds[i]
                rows.append((x_off, n, o_off, y_off, S, 0))
                parts += [wavs[i].reshape(-1), pad[: -n % 4]]
                x_off += n + (-n % 4)
                o_off += (frames(n, S) + 3) & ~3
                y_off += (out_len(n, S) + 3) & ~3
            x = torch.cat(parts)
            offsets = torch.empty(o_off, dtype=torch.int32, device=self.device)
            y = torch.empty(y_off, dtype=torch.float32, device=self.device)
            arr, raw = natm.table(rows)
            dev = natm.upload(raw, self.device)
            natm.search(x, offsets, arr, dev.data_ptr())
            natm.overlap_add(x, offsets, y, self._window, arr, dev.data_ptr())
            with self._lock:
                self.launches += 2
            for i, (_, n, o, yo, S, _) in zip(live, rows):
                outs[i], lags[i] = y[yo: yo + out_len(n, S)], offsets[o: o + frames(n, S)]
        if offsets_out is not None:
            offsets_out[:] = lags
        return outs

    @staticmethod
    def plan(pitch, speed):
        """(S, step) of one row: what process() and resample() are given for it.  pitch None or 0: (the row's speed as S, or None,
        and no step) -- exactly the speed= path; otherwise pitch_plan's WSOLA rate as S and its step."""
        if pitch is None or (not isinstance(pitch, bool) and isinstance(pitch, (int, float, np.integer, np.floating)) and pitch == 0):
            return (None if speed is None else fixed_speed(speed)), None
        rate, step, _ = pitch_plan(pitch, speed)
        return fixed_speed(rate), step

    def _table(self):
        with self._lock:
            if self._taps is None:                           # written once, at the first shift
                natr.lib()
                self._taps = ratio_table().to(self.device)
            return self._taps

    @torch.no_grad()
    def resample(self, wavs, steps):
        """wavs: fp32 device tensors [N_i]; steps: one per row -- None, or p in 32.32 fixed point (pitch_plan).  Returns their forms
        read at m p, fp32 device tensors [ceil(N_i 2^32 / step_i)], each bit-equal to that row resampled alone: ONE launch of
        ittr_resample_ratio for any number of rows.  A row at None or at 2^32, and a row without samples, comes back as the same
        tensor object."""
        wavs = [self._wave(w) for w in wavs]
        if len(steps) != len(wavs):
            raise ValueError(f"TempoEngine.resample: {len(steps)} steps for {len(wavs)} rows")
        for st in steps:
            if st is not None and (isinstance(st, bool) or not isinstance(st, (int, np.integer)) or not natr.STEP_MIN <= st <= natr.STEP_MAX):
                raise ValueError(f"step = {st!r} (an integer in [2^31, 2^33]: pitch_plan(semitones, speed)[1])")
        live = [i for i, (w, st) in enumerate(zip(wavs, steps)) if st is not None and st != STEP_ONE and w.numel()]
        outs = list(wavs)
        if live:
            pad = torch.zeros(3, dtype=torch.float32, device=self.device)
            parts, rows, x_off, y_off = [], [], 0, 0
            for i in live:                                   # every row starts at a multiple of 4 elements (16 bytes)
                n, st = int(wavs[i].numel()), int(steps[i])
                n_out = -((-n * STEP_ONE) // st)
                rows.append((x_off, n, y_off, n_out, st, cutoff_of(st), 0))
                parts += [wavs[i].reshape(-1), pad[: -n % 4]]
                x_off += n + (-n % 4)
                y_off += (n_out + 3) & ~3
            x = torch.cat(parts)
            y = torch.empty(y_off, dtype=torch.float32, device=self.device)
            arr, raw = natr.table(rows)
            dev = natm.upload(raw, self.device)
            natr.resample_ratio(x, y, self._table(), arr, dev.data_ptr())
            with self._lock:
                self.launches += 1
            for i, (_, _, yo, n_out, _, _, _) in zip(live, rows):
                outs[i] = y[yo: yo + n_out]
        return outs

    def shift(self, rows, lengths=None, pitch=None, speed=None):
        """rows: fp32 device tensors [N_i] (whole utterances at 24 kHz); lengths: None, or the samples of each row that count (the
        row is cut there); pitch: semitones, one number for all rows or one entry per row (None and 0: the pitch as it is);
        speed: likewise (None and 1.0: the duration as it is).  Returns every row at its pitch and speed: the two launches of
        process() at speed / p and the one of resample() by p, for any number of rows; a row with neither comes back as the same
        tensor, and a call where no row has either launches nothing.  A row's bits are those of the row shifted alone.  Every
        refusal (pitch_plan, fixed_speed, a list of another length) is a ValueError raised before any launch."""
        rows = list(rows)
        n = len(rows)

        def per_row(v, what):
            if isinstance(v, (list, tuple)):
                if len(v) != n:
                    raise ValueError(f"TempoEngine.shift: {len(v)} {what} for {n} rows")
                return list(v)
            return [v] * n

        plans = [self.plan(p, s) for p, s in zip(per_row(pitch, "pitches"), per_row(speed, "speeds"))]
        if lengths is not None:
            rows = [w[: int(k)] for w, k in zip(rows, per_row(list(lengths), "lengths"))]
        return self.shift_planned(rows, plans)

    def shift_planned(self, rows, plans):
        """shift() over plan()'s pairs."""
        return self.resample(self.process(rows, [S for S, _ in plans]), [step for _, step in plans])
