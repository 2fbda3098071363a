"""ctypes binding of libindextts_out.so (the C ABI declared in include/indextts_out.h): the PCM output back-end.

A library of its own beside libindextts_hip.so, libindextts_voice.so and libindextts_audio.so, loaded the same way: no
CPU/PyTorch fallback -- if the shared library is missing or a call fails, an exception is raised.  torch is used here only for
device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_out.so")
ABI_VERSION = 1                                     # ITTO_ABI_VERSION
SRC_RATE = 24000                                    # ITTO_SRC_RATE
MAX_TAP_BYTES = 1 << 20                             # ITTO_MAX_TAP_BYTES
WINDOW = 8192                                       # ITTO_WINDOW
RUN = 1024                                          # ITTO_RUN
ENCODINGS = {"f32": 0, "pcm16": 1, "mulaw": 2, "alaw": 3}                  # ITTO_ENC_*
DTYPES = {"f32": torch.float32, "pcm16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}


class Seg(C.Structure):
    """itto_seg (include/indextts_out.h)."""
    _fields_ = [("x_off", C.c_int64), ("y_off", C.c_int64), ("x0", C.c_int64), ("n_in", C.c_int64), ("N_total", C.c_int64),
                ("j0", C.c_int64), ("j1", C.c_int64), ("reserved", C.c_int64)]


class PcmOutArgs(C.Structure):
    """itto_pcm_out_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("y", C.c_void_p), ("y_elems", C.c_int64), ("kern_t", C.c_void_p),
                ("orig", C.c_int), ("new_", C.c_int), ("width", C.c_int), ("taps", C.c_int), ("encoding", C.c_int), ("n_seg", C.c_int),
                ("segs", C.POINTER(Seg)), ("segs_dev", C.c_void_p)]


_SIGNATURES = {
    "itto_abi_version": (C.c_int, []),
    "itto_last_error": (C.c_char_p, []),
    "itto_pcm_out": (C.c_int, [C.POINTER(PcmOutArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_out.h declares
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
        if L.itto_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_out.so ABI version mismatch")
        _lib = L
    return _lib


def seg_table(rows):
    """(the host array of Seg built from `rows` of field tuples, the same bytes as a CPU uint8 tensor to upload)."""
    arr = (Seg * len(rows))(*[Seg(*r) for r in rows])
    return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)


def pcm_out(x: torch.Tensor, y: torch.Tensor, kern_t: torch.Tensor | None, orig: int, new: int, width: int, encoding: str, segs,
            segs_dev: torch.Tensor):
    """Polyphase sinc and encoding of the pieces `segs` names (a host array of Seg; segs_dev the same bytes on the device) in one
    launch: fp32 samples at 24 kHz in x, the encoded samples into y (itto_pcm_out).  kern_t [taps, new] fp32 (the tap table
    transposed), or None with orig = new = 1 for the encoding alone."""
    for t in (x, y, kern_t, segs_dev):
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise NativeError("itto_pcm_out: needs contiguous device tensors (no CPU fallback)")
    if encoding not in ENCODINGS:
        raise NativeError(f"itto_pcm_out: encoding {encoding!r} is none of {sorted(ENCODINGS)}")
    if x.dtype != torch.float32 or y.dtype != DTYPES[encoding] or (kern_t is not None and (kern_t.dtype != torch.float32 or kern_t.dim() != 2)):
        raise NativeError(f"itto_pcm_out: x and kern_t are fp32 (kern_t [taps, new]), y is {DTYPES[encoding]} for {encoding}")
    if kern_t is not None and kern_t.shape[1] != new or segs_dev.numel() != C.sizeof(Seg) * len(segs):
        raise NativeError("itto_pcm_out: kern_t is [taps, new] and segs_dev holds the bytes of segs")
    a = PcmOutArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.kern_t = _p(x), x.numel(), _p(y), y.numel(), _p(kern_t)
    a.orig, a.new_, a.width, a.taps = int(orig), int(new), int(width), 0 if kern_t is None else int(kern_t.shape[0])
    a.encoding, a.n_seg, a.segs, a.segs_dev = ENCODINGS[encoding], len(segs), segs, _p(segs_dev)
    rc = lib().itto_pcm_out(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"itto_pcm_out failed (code {rc}): {lib().itto_last_error().decode()}")
    return y
