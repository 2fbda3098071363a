"""PCM output back-end on the device: the vocoder's fp32 samples at 24 kHz (int16 range, as _vocode leaves them) -> any sample
rate -> float / PCM16 / G.711, for one utterance, a ragged batch, or the rows of one stream boundary, in ONE itto_pcm_out launch
(libindextts_out.so, include/indextts_out.h).

The statement the resampler is held to is feature_extractors.resample(x, 24000, rate); the tap table is built here in float64 by
that formula and rounded once to fp32.  The plan, the table, its packed form and the stream planner are plain host functions, so
that the tests can hold them to that statement without a GPU.
"""
from __future__ import annotations

import functools
import math
import threading

import numpy as np
import torch

from indextts import _native_out as nato

SRC_RATE = nato.SRC_RATE
ENCODINGS = tuple(nato.ENCODINGS)
WAV_TAGS = {"pcm16": 1, "f32": 3, "alaw": 6, "mulaw": 7}          # WAVE_FORMAT_PCM / IEEE_FLOAT / ALAW / MULAW
MIME = {"pcm16": "audio/L16", "mulaw": "audio/PCMU", "alaw": "audio/PCMA", "f32": "audio/L32F"}
NUMPY = {"f32": "<f4", "pcm16": "<i2", "mulaw": "u1", "alaw": "u1"}


def out_plan(rate: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(orig, new, width, taps) of feature_extractors.resample(., 24000, rate); (1, 1, 0, 0) at 24 kHz."""
    rate = int(rate)
    if rate <= 0:
        raise ValueError(f"sample rate {rate}")
    if rate == SRC_RATE:
        return 1, 1, 0, 0
    g = math.gcd(SRC_RATE, rate)
    orig, new = SRC_RATE // g, rate // g
    width = math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))
    return orig, new, width, 2 * width + orig


def out_len(n: int, rate: int) -> int:
    orig, new, _, _ = out_plan(rate)
    return -(-new * int(n) // orig)


def refusal(rate):
    """Why libindextts_out.so does not produce `rate`, or None."""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) <= 0:
        return f"sample rate {rate!r}: a positive integer"
    orig, new, _, taps = out_plan(rate)
    if new * taps * 4 > nato.MAX_TAP_BYTES:
        return f"sample rate {rate} needs a tap table of {new} x {taps} fp32 = {new * taps * 4} bytes (at most {nato.MAX_TAP_BYTES})"
    if 4 * orig + taps > nato.WINDOW:
        return f"sample rate {rate} needs a window of {4 * orig + taps} samples (at most {nato.WINDOW})"
    return None


@functools.lru_cache(maxsize=32)
def tap_table(rate: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """The `kern` feature_extractors.resample builds for 24000 -> rate, float64 rounded once to fp32: [new, taps].  (Shared
    between callers: do not write to it.)"""
    why = refusal(rate)
    if why is not None or int(rate) == SRC_RATE:
        raise ValueError(why or "24 kHz has no tap table")
    orig, new, width, _ = out_plan(rate, lowpass_filter_width, rolloff)
    base = min(orig, new) * rolloff
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return kern.to(torch.float32).contiguous()


def pack_taps(kern: torch.Tensor) -> torch.Tensor:
    """The layout itto_pcm_out reads (include/indextts_out.h): [taps][new], phase-minor, so that the lanes of one wave -- one
    output, hence one phase, each -- read one tap of neighbouring phases at neighbouring addresses."""
    return kern.t().contiguous()


class OutputFormat:
    """What the caller wants the samples as: sample_rate (a positive integer the library has a table for) and encoding
    ("pcm16", "f32", "mulaw", "alaw").  OutputFormat() is what the build has always produced: 24 kHz PCM16."""
    __slots__ = ("sample_rate", "encoding")

    def __init__(self, sample_rate: int = SRC_RATE, encoding: str = "pcm16"):
        why = refusal(sample_rate)
        if why is not None:
            raise ValueError(f"OutputFormat: {why}")
        if encoding not in nato.ENCODINGS:
            raise ValueError(f"OutputFormat: encoding {encoding!r} is none of {list(nato.ENCODINGS)}")
        object.__setattr__(self, "sample_rate", int(sample_rate))
        object.__setattr__(self, "encoding", encoding)

    def __setattr__(self, *_):
        raise AttributeError("an OutputFormat does not change")

    def __eq__(self, other):
        return isinstance(other, OutputFormat) and (self.sample_rate, self.encoding) == (other.sample_rate, other.encoding)

    def __hash__(self):
        return hash((self.sample_rate, self.encoding))

    def __repr__(self):
        return f"OutputFormat(sample_rate={self.sample_rate}, encoding={self.encoding!r})"

    @property
    def dtype(self):
        return nato.DTYPES[self.encoding]

    @property
    def bytes_per_sample(self):
        return {"f32": 4, "pcm16": 2}.get(self.encoding, 1)

    @property
    def wav_tag(self):
        return WAV_TAGS[self.encoding]

    @property
    def content_type(self):
        return f"{MIME[self.encoding]}; rate={self.sample_rate}"

    def to_bytes(self, pcm: torch.Tensor) -> bytes:
        """An encoded chunk as the little-endian bytes that go on the wire or into a file."""
        return pcm.cpu().numpy().astype(NUMPY[self.encoding], copy=False).tobytes()


class StreamPlan:
    """The host side of one utterance's stream: which outputs each push determines and which input samples are carried.
    A non-final push emits exactly the outputs j = q new + p whose whole support [q orig - width, q orig + width + orig) has
    arrived; the final one emits up to out_len(N).  Between two pushes the samples from `x0` on are kept: the first sample the
    next output reads, fewer than taps of them."""

    def __init__(self, rate):
        self.orig, self.new, self.width, self.taps = out_plan(rate)
        self.arrived = 0        # input samples seen
        self.emitted = 0        # outputs given out
        self.x0 = 0             # the absolute index of the first carried sample
        self.closed = False

    def advance(self, n_chunk: int, last: bool):
        """n_chunk more samples have arrived (last: and the utterance ends with them).  Returns dict(x0, n_in, N_total, j0, j1):
        the samples [x0, x0 + n_in) -- the carried tail, then the chunk -- give the outputs [j0, j1); afterwards the samples from
        self.x0 on are carried."""
        if self.closed:
            raise ValueError("PcmOutStream: the utterance has had its last chunk")
        n_chunk = int(n_chunk)
        if n_chunk < 0:
            raise ValueError("PcmOutStream: a chunk holds no fewer than 0 samples")
        self.arrived += n_chunk
        x0, j0 = self.x0, self.emitted
        if last:
            j1 = -(-self.new * self.arrived // self.orig)
            self.closed = True
        else:
            ready = (self.arrived - self.width - self.orig) // self.orig + 1        # the q whose support is complete
            j1 = max(j0, self.new * max(0, ready))
        self.emitted = j1
        # (every emitted count but the last is a multiple of new: the next output is phase 0 of q = j1 / new)
        self.x0 = min(self.arrived, max(x0, (j1 // self.new) * self.orig - self.width))
        return dict(x0=x0, n_in=self.arrived - x0, N_total=self.arrived if last else -1, j0=j0, j1=j1)


class PcmOutStream:
    """One utterance's streaming state: push(chunk, last) returns the newly determined output samples; the concatenation of the
    pushes is, bit for bit, PcmOutEngine.encode of the whole utterance.  The carried tail (fewer than taps samples) stays on the
    device."""

    def __init__(self, engine: "PcmOutEngine", fmt: OutputFormat):
        self.engine, self.fmt, self.plan, self.tail = engine, fmt, StreamPlan(fmt.sample_rate), None

    def push(self, chunk: torch.Tensor, last: bool = False) -> torch.Tensor:
        return self.engine.push_many([(self, chunk, last)])[0]


class PcmOutEngine:
    """encode(waves, fmt) / push_many(rows): one itto_pcm_out launch for any number of rows.  Owns the packed tap tables on
    `device` (one per rate seen, guarded by a lock); every call works on tensors of its own, so one engine may serve several
    threads and a result is never overwritten by a later call."""
    MAX_TAP_TABLES = 16

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        nato.lib()
        self._taps = {}
        self._lock = threading.Lock()
        self.launches = 0

    def taps(self, rate):
        """The packed table of `rate` on the device (None at 24 kHz)."""
        if int(rate) == SRC_RATE:
            return None
        with self._lock:
            t = self._taps.get(rate)
            if t is None:
                if len(self._taps) >= self.MAX_TAP_TABLES:
                    self._taps.clear()
                t = self._taps[rate] = pack_taps(tap_table(int(rate))).to(self.device)
            return t

    def stream(self, fmt: OutputFormat) -> PcmOutStream:
        return PcmOutStream(self, fmt)

    def _wave(self, w):
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != self.device:
            raise ValueError(f"PcmOutEngine: a waveform is an fp32 tensor on {self.device} (the vocoder's samples, int16 range)")
        return w.reshape(-1)

    @staticmethod
    def _cat(pieces):
        pieces = [p for p in pieces if p.numel()]
        return None if not pieces else pieces[0].contiguous() if len(pieces) == 1 else torch.cat(pieces)

    def _launch(self, fmt, x, rows):
        """x: the fp32 samples of the launch (None: there are none); rows: (x_off, x0, n_in, N_total, j0, j1).  Returns one
        output tensor per row."""
        y_off, table = 0, []
        for x_off, x0, n_in, N_total, j0, j1 in rows:
            table.append((x_off, y_off, x0, n_in, N_total, j0, j1, 0))
            y_off += (j1 - j0 + 3) & ~3
        y = torch.empty(y_off, dtype=fmt.dtype, device=self.device)
        if y_off:                 # (an output needs at least one sample: x is there)
            arr, raw = nato.seg_table(table)
            orig, new, width, _ = out_plan(fmt.sample_rate)
            nato.pcm_out(x, y, self.taps(fmt.sample_rate), orig, new, width, fmt.encoding, arr, raw.to(self.device))
            with self._lock:
                self.launches += 1
        return [y[r[1]: r[1] + r[6] - r[5]] for r in table]

    @torch.no_grad()
    def encode(self, waves, fmt: OutputFormat):
        """waves: fp32 device tensors [N_i] (whole utterances at 24 kHz).  Returns the list of their encoded forms, device
        tensors [out_len(N_i)] of fmt.dtype; each is bit-equal to that row encoded alone."""
        waves = [self._wave(w) for w in waves]
        rows, off = [], 0
        for w in waves:
            n = int(w.numel())
            rows.append((off, 0, n, n, 0, out_len(n, fmt.sample_rate)))
            off += n
        return self._launch(fmt, self._cat(waves), rows)

    @torch.no_grad()
    def push_many(self, items):
        """items: [(stream, chunk, last)] -- the rows of one stream boundary, every stream of this engine and of one format.
        ONE launch; returns each row's newly determined samples, in order."""
        if not items:
            return []
        fmt = items[0][0].fmt
        if any(s.engine is not self or s.fmt != fmt for s, _, _ in items) or len({id(s) for s, _, _ in items}) != len(items):
            raise ValueError("PcmOutEngine.push_many: distinct streams of this engine and of one output format")
        chunks = [self._wave(c) for _, c, _ in items]
        if any(s.plan.closed for s, _, _ in items):
            raise ValueError("PcmOutStream: the utterance has had its last chunk")
        pieces, rows, spans, off = [], [], [], 0
        for (s, _, last), c in zip(items, chunks):
            tail = s.tail if s.tail is not None else c[:0]
            p = s.plan.advance(int(c.numel()), bool(last))
            assert p["n_in"] == int(tail.numel()) + int(c.numel())
            pieces += [tail, c]
            rows.append((off, p["x0"], p["n_in"], p["N_total"], p["j0"], p["j1"]))
            spans.append((off + s.plan.x0 - p["x0"], off + p["n_in"]))
            off += p["n_in"]
        x = self._cat(pieces)
        outs = self._launch(fmt, x, rows)
        for (s, _, last), (a, b) in zip(items, spans):
            s.tail = None if last or x is None or b <= a else x[a:b].clone()
        return outs
