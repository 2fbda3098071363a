"""Prompt audio front-end on the device: decoded waveform -> mono -> 24 kHz -> log-mel [1, 100, T], for one prompt or a ragged
batch of prompts, in one itta_resample launch per distinct sample rate and one itta_logmel launch (libindextts_audio.so,
include/indextts_audio.h).

The statement this is held to is feature_extractors.py (resample, MelSpectrogramFeatures), which stays the default path.  The
host tables -- polyphase taps, the windowed cosine / sine bases, the mel filterbank and its bin ranges -- are plain functions
here, built in float64 and rounded once to fp32, so that the tests can hold them to that statement without a GPU.
"""
from __future__ import annotations

import math
import threading

import numpy as np
import torch

from indextts import _native_audio as nata
from indextts.utils.feature_extractors import mel_filterbank

TARGET_SR = 24000
N_FFT, HOP, N_BINS, N_MELS = nata.N_FFT, nata.HOP, nata.N_BINS, nata.N_MELS


class PromptAudioRefused(ValueError):
    """An input the device front-end does not take (IndexTTS sends such a file through the torch path, with a warning)."""


def resample_plan(sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(orig, new, width, taps) of feature_extractors.resample(., sr, 24000); (1, 1, 0, 0) at 24 kHz."""
    sr = int(sr)
    if sr <= 0:
        raise PromptAudioRefused(f"sample rate {sr}")
    if sr == TARGET_SR:
        return 1, 1, 0, 0
    g = math.gcd(sr, TARGET_SR)
    orig, new = sr // g, TARGET_SR // g
    width = math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))
    return orig, new, width, 2 * width + orig


def tap_table(sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """The `kern` feature_extractors.resample builds for sr -> 24000, float64 rounded once to fp32: [new, taps]."""
    orig, new, width, taps = resample_plan(sr, lowpass_filter_width, rolloff)
    if new * taps * 4 > nata.MAX_TAP_BYTES:
        raise PromptAudioRefused(f"sample rate {sr}: a tap table of {new} x {taps} fp32 is above {nata.MAX_TAP_BYTES} bytes")
    base = min(orig, new) * rolloff
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return kern.to(torch.float32).contiguous()


def resampled_len(n: int, sr: int) -> int:
    orig, new, _, _ = resample_plan(sr)
    return -(-new * int(n) // orig)


def frame_count(n: int) -> int:
    return 1 + int(n) // HOP


def dft_bases64():
    """(cos, sin) [1024, 513] float64 with the periodic Hann window folded in: frames @ cos, frames @ sin are re, -im of the STFT."""
    k = torch.arange(N_FFT, dtype=torch.int64)[:, None]
    f = torch.arange(N_BINS, dtype=torch.int64)[None]
    ang = ((k * f) % N_FFT).to(torch.float64) * (2.0 * math.pi / N_FFT)      # the angle reduced exactly, in integers
    win = 0.5 - 0.5 * torch.cos(torch.arange(N_FFT, dtype=torch.float64) * (2.0 * math.pi / N_FFT))
    return win[:, None] * torch.cos(ang), win[:, None] * torch.sin(ang)


def dft_bases():
    """The two bases rounded once to fp32."""
    c, s = dft_bases64()
    return c.to(torch.float32), s.to(torch.float32)


def pack_basis(cos32: torch.Tensor, sin32: torch.Tensor) -> torch.Tensor:
    """The layout itta_logmel reads (include/indextts_audio.h): [33 bin tiles][64 k-steps][cos, sin][lane = 16 g + c][j] with
    k = 16 ks + 4 g + j and bin = 16 nt + c, zeros past bin 512."""
    both = torch.zeros(2, N_FFT, nata.BIN_TILES * 16, dtype=torch.float32)
    both[0, :, :N_BINS], both[1, :, :N_BINS] = cos32, sin32
    p = both.reshape(2, 64, 4, 4, nata.BIN_TILES, 16).permute(4, 1, 0, 2, 5, 3)     # cs ks g j nt c -> nt ks cs g c j
    return p.contiguous().reshape(-1)


def mel_tables():
    """(fb [513, 100] fp32 as MelSpectrogramFeatures holds it, fb_t [100, 513], rng int32 [100, 2]: mel m's nonzero bins are
    [lo, hi), an empty mel has lo == hi)."""
    fb = mel_filterbank(N_BINS, 0.0, float(TARGET_SR // 2), N_MELS, TARGET_SR)
    rng = torch.zeros(N_MELS, 2, dtype=torch.int32)
    for m in range(N_MELS):
        nz = torch.nonzero(fb[:, m]).flatten()
        if nz.numel():
            lo, hi = int(nz[0]), int(nz[-1]) + 1
            assert nz.numel() == hi - lo, "a mel triangle is one run of bins"
            rng[m, 0], rng[m, 1] = lo, hi
    return fb, fb.t().contiguous(), rng


def as_planar(audio) -> torch.Tensor:
    """An array / tensor [N] or [C, N] -> an fp32 CPU tensor [C, N] (a view where it can be: the engine's staging copy is the
    one pass that lays the samples out)."""
    t = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio))
    t = t.detach().to("cpu", torch.float32)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise PromptAudioRefused(f"a waveform is [N] or [C, N] with at least one channel and one sample (got {tuple(t.shape)})")
    return t


def _up4(n):
    return (n + 3) & ~3


def refusal(shape, sr):
    """Why the engine does not take a wave of `shape` (C, N) at rate `sr` -- every condition libindextts_audio.so would refuse
    it for -- or None."""
    c, n, sr = int(shape[0]), int(shape[1]), int(sr)
    if sr <= 0:
        return f"sample rate {sr}"
    if not 1 <= c <= nata.MAX_CHANNELS:
        return f"{c} channels (1 to {nata.MAX_CHANNELS})"
    if n < 1:
        return "no samples"
    _, new, _, taps = resample_plan(sr)
    if new * taps * 4 > nata.MAX_TAP_BYTES:
        return f"sample rate {sr} needs a tap table of {new * taps * 4} bytes (at most {nata.MAX_TAP_BYTES})"
    n_out = resampled_len(n, sr)
    if n_out <= N_FFT // 2:
        return f"{n_out} samples at 24 kHz; the reflect padding needs more than {N_FFT // 2}"
    if n_out >= 1 << 30 or c * n >= 1 << 31:
        return f"{n} samples ({n_out} at 24 kHz): one prompt holds fewer than 2^30"
    return None


def segment_plan(shapes, rates):
    """The layout of one engine pass.  shapes: (C, N) per wave.  Returns dict(x_elems, y_elems, frames, waves=[dict(C, N, sr,
    x_off, y_off, n_out, T, frame_off)], groups={sr: [wave indices]}): planar inputs and mono outputs packed one after the other
    at offsets that are multiples of 4 elements, the mels packed frame after frame."""
    waves, groups, x_off, y_off, frame_off = [], {}, 0, 0, 0
    for i, ((c, n), sr) in enumerate(zip(shapes, rates)):
        c, n, sr = int(c), int(n), int(sr)
        why = refusal((c, n), sr)
        if why is not None:
            raise PromptAudioRefused(f"wave {i}: {why}")
        n_out = resampled_len(n, sr)
        T = frame_count(n_out)
        waves.append(dict(C=c, N=n, sr=sr, x_off=x_off, y_off=y_off, n_out=n_out, T=T, frame_off=frame_off))
        groups.setdefault(sr, []).append(i)
        x_off, y_off, frame_off = x_off + _up4(c * n), y_off + _up4(n_out), frame_off + T
    return dict(x_elems=x_off, y_elems=y_off, frames=frame_off, waves=waves, groups=groups)


class PromptAudioEngine:
    """mel(waves, rates): the log-mels of any number of decoded waveforms in one pass.  Owns the tap tables (one per sample rate
    seen), the two bases, the filterbank and its ranges on `device`, and per thread a bounded cache of the staging buffers.
    Independent of the model's dtype: the kernels are fp32.  One engine may serve several threads (the replicas of a RequestPool
    share it): the staging buffers are per thread, the tap tables and the launch counter are guarded by a lock."""
    MAX_CACHED_BYTES = 64 << 20      # staging buffers above this are allocated for the call and not kept
    MAX_TAP_TABLES = 16

    def __init__(self, device):
        self.device = torch.device(device)
        nata.lib()
        self.basis = pack_basis(*dft_bases()).to(self.device)
        _, fb_t, rng = mel_tables()
        self.fb_t, self.mel_rng = fb_t.to(self.device), rng.to(self.device)
        self._taps = {}
        self._lock = threading.Lock()
        self._local = threading.local()
        self.launches = 0

    def forget(self):
        """Drop this thread's staging buffers and every tap table (the bases and the filterbank stay)."""
        self._local.bufs = {}
        with self._lock:
            self._taps.clear()

    @property
    def _bufs(self):
        b = getattr(self._local, "bufs", None)
        if b is None:
            b = self._local.bufs = {}
        return b

    def _buf(self, name, n, dtype, host=False):
        """n elements of `dtype` on the device (host=True: in pinned host memory), reused from call to call while they stay
        under the bound.  A copy out of a pinned buffer below is a blocking one, so the buffer is free again when it returns."""
        t = self._bufs.get(name)
        if t is not None and t.numel() >= n:
            return t
        size = max(1024, 1 << (int(n) - 1).bit_length())
        t = torch.empty(size, dtype=dtype, pin_memory=True) if host else torch.empty(size, dtype=dtype, device=self.device)
        if t.numel() * t.element_size() <= self.MAX_CACHED_BYTES:
            self._bufs[name] = t
        else:
            self._bufs.pop(name, None)
        return t

    def taps(self, sr):
        with self._lock:
            t = self._taps.get(sr)
            if t is None:
                if len(self._taps) >= self.MAX_TAP_TABLES:
                    self._taps.clear()
                t = self._taps[sr] = tap_table(sr).to(self.device)
            return t

    @torch.no_grad()
    def mel(self, waves, rates):
        """waves: arrays / tensors [N] or [C, N] (decoded, any float type; host or device); rates: their sample rates.  Returns a
        list of [1, 100, T_i] fp32 device tensors.  A prompt's mel is bit-equal whatever else is in the pass."""
        if len(waves) != len(rates) or not len(waves):
            raise ValueError("PromptAudioEngine.mel: one sample rate per waveform, at least one waveform")
        planar = [as_planar(w) for w in waves]
        plan = segment_plan([tuple(p.shape) for p in planar], rates)
        hx = self._buf("hx", plan["x_elems"], torch.float32, host=True)[:plan["x_elems"]]
        for p, w in zip(planar, plan["waves"]):       # the one host pass over the samples: layout (and dtype) into pinned memory
            hx[w["x_off"]:w["x_off"] + p.numel()].view(p.shape).copy_(p)
        # every segment table of the pass in one upload: a resample table per rate, then the log-mel table (16-byte slots)
        tables, blobs, off = [], [], 0
        for sr, idx in plan["groups"].items():
            arr, raw = nata.seg_table(nata.WaveSeg, [(plan["waves"][i]["x_off"], plan["waves"][i]["y_off"], plan["waves"][i]["C"],
                                                      plan["waves"][i]["N"], plan["waves"][i]["n_out"], 0) for i in idx])
            tables.append((sr, arr, off, raw.numel()))
            blobs.append(raw)
            off += raw.numel()
        marr, mraw = nata.seg_table(nata.MelSeg, [(w["y_off"], w["frame_off"], w["n_out"], w["T"]) for w in plan["waves"]])
        m_off = off
        blobs.append(mraw)
        hseg = torch.cat(blobs)
        x = self._buf("x", plan["x_elems"], torch.float32)
        y = self._buf("y", plan["y_elems"], torch.float32)
        segs = self._buf("segs", hseg.numel(), torch.uint8)
        x[:hx.numel()].copy_(hx)
        segs[:hseg.numel()].copy_(hseg)
        for sr, arr, o, nb in tables:
            orig, new, width, _ = resample_plan(sr)
            nata.resample(x, y, None if sr == TARGET_SR else self.taps(sr), orig, new, width, arr, segs[o:o + nb])
        out = torch.empty(N_MELS * plan["frames"], dtype=torch.float32, device=self.device)
        nata.logmel(y, out, self.basis, self.fb_t, self.mel_rng, marr, segs[m_off:m_off + mraw.numel()])
        with self._lock:
            self.launches += len(tables) + 1
        return [out[N_MELS * w["frame_off"]:N_MELS * (w["frame_off"] + w["T"])].view(1, N_MELS, w["T"]) for w in plan["waves"]]
