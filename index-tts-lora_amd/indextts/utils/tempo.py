"""The speaking rate on the device, between the vocoder's fp32 samples (24 kHz, int16 range, as _vocode leaves them) and waveform
finishing: WSOLA time-scale modification (libindextts_tempo.so, include/indextts_tempo.h).  24 kHz fp32
goes in and the same comes out, shorter or longer, at the same pitch; so it composes with post= and with every OutputFormat.

Two launches for any number of rows: ittm_search (the chain of lags of every row, one workgroup per row) and ittm_overlap_add.
The lengths are plain integer arithmetic, so that the tests can hold them to their own restatement without a GPU.
"""
from __future__ import annotations

import math
import threading

import numpy as np
import torch

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


class TempoEngine:
    """process(wavs, speeds): ittm_search and ittm_overlap_add -- two launches for any number of rows.  Owns the window on
    `device` (written once) and nothing else that is shared: the sample, lag, table and output tensors of a call are that call's
    own, so one engine may serve several threads and a result is never overwritten by a later call."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        natm.lib()
        self._window = window_table().to(self.device)
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
