"""ctypes binding of libindextts_audio.so (the C ABI declared in include/indextts_audio.h): the prompt audio front-end.

A library of its own beside libindextts_hip.so and libindextts_voice.so, loaded the same way: no CPU/PyTorch fallback -- if the
shared library is missing or a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_audio.so")
ABI_VERSION = 1                                     # ITTA_ABI_VERSION
MAX_CHANNELS = 8                                    # ITTA_MAX_CHANNELS
MAX_TAP_BYTES = 1 << 20                             # ITTA_MAX_TAP_BYTES
N_FFT, HOP, N_BINS, N_MELS, BIN_TILES = 1024, 256, 513, 100, 33
BASIS_ELEMS = BIN_TILES * 64 * 2 * 64 * 4           # ITTA_BASIS_ELEMS


class WaveSeg(C.Structure):
    """itta_wave_seg (include/indextts_audio.h)."""
    _fields_ = [("x_off", C.c_int64), ("y_off", C.c_int64), ("C", C.c_int32), ("N", C.c_int32), ("n_out", C.c_int32),
                ("reserved", C.c_int32)]


class ResampleArgs(C.Structure):
    """itta_resample_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("y", C.c_void_p), ("y_elems", C.c_int64), ("kern", C.c_void_p),
                ("orig", C.c_int), ("new_", C.c_int), ("width", C.c_int), ("taps", C.c_int),
                ("segs", C.POINTER(WaveSeg)), ("segs_dev", C.c_void_p), ("n_seg", C.c_int)]


class MelSeg(C.Structure):
    """itta_mel_seg."""
    _fields_ = [("sample_off", C.c_int64), ("frame_off", C.c_int64), ("N", C.c_int32), ("T", C.c_int32)]


class LogmelArgs(C.Structure):
    """itta_logmel_args."""
    _fields_ = [("wave", C.c_void_p), ("wave_elems", C.c_int64), ("out", C.c_void_p), ("out_elems", C.c_int64),
                ("basis", C.c_void_p), ("fb_t", C.c_void_p), ("mel_rng", C.c_void_p),
                ("segs", C.POINTER(MelSeg)), ("segs_dev", C.c_void_p), ("n_seg", C.c_int)]


_SIGNATURES = {
    "itta_abi_version": (C.c_int, []),
    "itta_last_error": (C.c_char_p, []),
    "itta_resample": (C.c_int, [C.POINTER(ResampleArgs), C.c_void_p]),
    "itta_logmel": (C.c_int, [C.POINTER(LogmelArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_audio.h declares
_lib = None


def lib():
    """Load (once) and return the shared library; raise NativeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} not found: build it with `make -C index-tts-lora_amd/csrc` "
                              f"(or python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.itta_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_audio.so ABI version mismatch")
        _lib = L
    return _lib


def seg_table(struct, rows):
    """(the host array of `struct` built from `rows` of field tuples, the same bytes as a CPU uint8 tensor to upload)."""
    arr = (struct * len(rows))(*[struct(*r) for r in rows])
    return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)


def _dev(who, *ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise NativeError(f"{who}: needs contiguous device tensors (no CPU fallback)")


def resample(x: torch.Tensor, y: torch.Tensor, kern: torch.Tensor | None, orig: int, new: int, width: int, segs, segs_dev: torch.Tensor):
    """Channel mean and polyphase sinc of the waves `segs` names (a host array of WaveSeg; segs_dev the same bytes on the device)
    in one launch: fp32 planar waves in x, their mono 24 kHz forms into y (itta_resample).  kern [new, taps] fp32, or None with
    orig = new = 1 for the channel mean alone."""
    _dev("itta_resample", x, y, kern, segs_dev)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or (kern is not None and (kern.dtype != torch.float32 or kern.dim() != 2)):
        raise NativeError("itta_resample: x, y and kern are fp32 (kern [new, taps])")
    a = ResampleArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.kern = _p(x), x.numel(), _p(y), y.numel(), _p(kern)
    a.orig, a.new_, a.width, a.taps = int(orig), int(new), int(width), 0 if kern is None else int(kern.shape[1])
    a.segs, a.segs_dev, a.n_seg = segs, _p(segs_dev), len(segs)
    if kern is not None and kern.shape[0] != new or segs_dev.numel() != C.sizeof(WaveSeg) * len(segs):
        raise NativeError("itta_resample: kern is [new, taps] and segs_dev holds the bytes of segs")
    rc = lib().itta_resample(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"itta_resample failed (code {rc}): {lib().itta_last_error().decode()}")
    return y


def logmel(wave: torch.Tensor, out: torch.Tensor, basis: torch.Tensor, fb_t: torch.Tensor, mel_rng: torch.Tensor, segs,
           segs_dev: torch.Tensor):
    """Log-mel of the prompts `segs` names (a host array of MelSeg; segs_dev the same bytes on the device) in one launch: 24 kHz
    mono fp32 samples in wave, every prompt's [100, T] contiguous into out (itta_logmel)."""
    _dev("itta_logmel", wave, out, basis, fb_t, mel_rng, segs_dev)
    if any(t.dtype != torch.float32 for t in (wave, out, basis, fb_t)) or mel_rng.dtype != torch.int32:
        raise NativeError("itta_logmel: wave, out, basis and fb_t are fp32, mel_rng int32")
    if basis.numel() != BASIS_ELEMS or tuple(fb_t.shape) != (N_MELS, N_BINS) or tuple(mel_rng.shape) != (N_MELS, 2) \
            or segs_dev.numel() != C.sizeof(MelSeg) * len(segs):
        raise NativeError("itta_logmel: basis holds ITTA_BASIS_ELEMS, fb_t is [100, 513], mel_rng [100, 2], segs_dev the bytes of segs")
    a = LogmelArgs()
    a.wave, a.wave_elems, a.out, a.out_elems = _p(wave), wave.numel(), _p(out), out.numel()
    a.basis, a.fb_t, a.mel_rng = _p(basis), _p(fb_t), _p(mel_rng)
    a.segs, a.segs_dev, a.n_seg = segs, _p(segs_dev), len(segs)
    rc = lib().itta_logmel(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"itta_logmel failed (code {rc}): {lib().itta_last_error().decode()}")
    return out
