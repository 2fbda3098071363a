"""ctypes binding of libindextts_post.so (the C ABI declared in include/indextts_post.h): waveform finishing.

A library of its own beside libindextts_hip.so, libindextts_voice.so, libindextts_audio.so and libindextts_out.so, loaded the
same way: no CPU/PyTorch fallback -- if the shared library is missing or a call fails, an exception is raised.  torch is used
here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_post.so")
ABI_VERSION = 1                                     # ITTP_ABI_VERSION
FRAME = 240                                         # ITTP_FRAME
FADE = 120                                          # ITTP_FADE
FRAMES_PER_WG = 16                                  # ITTP_FRAMES_PER_WG
RUN = 1024                                          # ITTP_RUN


class Row(C.Structure):
    """ittp_row (include/indextts_post.h)."""
    _fields_ = [("x_off", C.c_int64), ("n", C.c_int64)]


class Piece(C.Structure):
    """ittp_piece."""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("n", C.c_int64), ("fade_in", C.c_int32), ("fade_out", C.c_int32)]


class OutRow(C.Structure):
    """ittp_out_row."""
    _fields_ = [("x_off", C.c_int64), ("n_in", C.c_int64), ("y_off", C.c_int64), ("n_out", C.c_int64), ("piece0", C.c_int32),
                ("n_pieces", C.c_int32), ("gain", C.c_float), ("reserved", C.c_int32)]


class FrameStatsArgs(C.Structure):
    """ittp_frame_stats_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("stats", C.c_void_p), ("stats_elems", C.c_int64), ("stat_stride", C.c_int64),
                ("n_rows", C.c_int), ("reserved", C.c_int), ("rows", C.POINTER(Row)), ("rows_dev", C.c_void_p)]


class SpliceArgs(C.Structure):
    """ittp_splice_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("y", C.c_void_p), ("y_elems", C.c_int64), ("ramp", C.c_void_p),
                ("n_rows", C.c_int), ("n_pieces", C.c_int), ("rows", C.POINTER(OutRow)), ("rows_dev", C.c_void_p),
                ("pieces", C.POINTER(Piece)), ("pieces_dev", C.c_void_p)]


_SIGNATURES = {
    "ittp_abi_version": (C.c_int, []),
    "ittp_last_error": (C.c_char_p, []),
    "ittp_frame_stats": (C.c_int, [C.POINTER(FrameStatsArgs), C.c_void_p]),
    "ittp_splice": (C.c_int, [C.POINTER(SpliceArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_post.h declares
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
        if L.ittp_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_post.so ABI version mismatch")
        _lib = L
    return _lib


def table(kind, rows):
    """(the host array of `kind` -- Row, Piece or OutRow -- built from `rows` of field tuples, its bytes)."""
    arr = (kind * len(rows))(*[kind(*r) for r in rows])
    return arr, bytes(arr)


def upload(*blobs, device):
    """The byte strings in ONE device tensor (one copy), each at a multiple of 16 bytes: (the tensor, their offsets)."""
    offs, buf = [], bytearray()
    for b in blobs:
        buf += b"\0" * (-len(buf) % 16)
        offs.append(len(buf))
        buf += b
    buf += b"\0" * (16 - len(buf) % 16)             # (never empty)
    return torch.frombuffer(buf, dtype=torch.uint8).to(device), offs


def _check(*tensors):
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise NativeError("libindextts_post.so needs contiguous device tensors (no CPU fallback)")


def frame_stats(x: torch.Tensor, stats: torch.Tensor, rows, rows_dev: int):
    """Sum of squares and peak of every ITTP_FRAME samples of the utterances `rows` names (a host array of Row; rows_dev the
    address of the same bytes on the device) of x (fp32) into stats [n_rows, stride, 2] fp32 (ittp_frame_stats)."""
    _check(x, stats)
    if x.dtype != torch.float32 or stats.dtype != torch.float32 or stats.dim() != 3 or stats.shape[0] != len(rows) or stats.shape[2] != 2:
        raise NativeError("ittp_frame_stats: x is fp32 and stats fp32 [n_rows, stride, 2]")
    a = FrameStatsArgs()
    a.x, a.x_elems, a.stats, a.stats_elems, a.stat_stride = _p(x), x.numel(), _p(stats), stats.numel(), int(stats.shape[1])
    a.n_rows, a.rows, a.rows_dev = len(rows), rows, rows_dev
    rc = lib().ittp_frame_stats(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittp_frame_stats failed (code {rc}): {lib().ittp_last_error().decode()}")
    return stats


def splice(x: torch.Tensor, y: torch.Tensor, ramp: torch.Tensor, rows, rows_dev: int, pieces, pieces_dev: int):
    """Gather, fade and scale: the pieces (a host array of Piece) of the output rows (a host array of OutRow) from x (fp32) into
    y (fp32) in one launch (ittp_splice); ramp fp32 [ITTP_FADE]; *_dev the addresses of the tables' bytes on the device."""
    _check(x, y, ramp)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or ramp.dtype != torch.float32 or ramp.numel() != FADE:
        raise NativeError(f"ittp_splice: x, y and ramp are fp32, ramp of {FADE} elements")
    a = SpliceArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.ramp = _p(x), x.numel(), _p(y), y.numel(), _p(ramp)
    a.n_rows, a.n_pieces, a.rows, a.rows_dev = len(rows), len(pieces), rows, rows_dev
    a.pieces, a.pieces_dev = (pieces, pieces_dev) if len(pieces) else (None, None)
    rc = lib().ittp_splice(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittp_splice failed (code {rc}): {lib().ittp_last_error().decode()}")
    return y
