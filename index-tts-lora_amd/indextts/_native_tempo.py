"""ctypes binding of libindextts_tempo.so (the C ABI declared in include/indextts_tempo.h): the speaking rate (WSOLA).

A library of its own beside libindextts_hip.so, libindextts_voice.so, libindextts_audio.so, libindextts_out.so and
libindextts_post.so, loaded the same way: no CPU/PyTorch fallback -- if the shared library is missing or a call fails, an
exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_tempo.so")
ABI_VERSION = 1                                     # ITTM_ABI_VERSION
HOP = 384                                           # ITTM_HOP
WIN = 768                                           # ITTM_WIN
TOL = 192                                           # ITTM_TOL
SPEED_ONE = 1024                                    # ITTM_SPEED_ONE
SPEED_MIN = 512                                     # ITTM_SPEED_MIN
SPEED_MAX = 2048                                    # ITTM_SPEED_MAX
RUN = 1024                                          # ITTM_RUN


class Row(C.Structure):
    """ittm_row (include/indextts_tempo.h)."""
    _fields_ = [("x_off", C.c_int64), ("n", C.c_int64), ("o_off", C.c_int64), ("y_off", C.c_int64), ("speed", C.c_int32),
                ("reserved", C.c_int32)]


class SearchArgs(C.Structure):
    """ittm_search_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("offsets", C.c_void_p), ("offsets_elems", C.c_int64), ("n_rows", C.c_int),
                ("reserved", C.c_int), ("rows", C.POINTER(Row)), ("rows_dev", C.c_void_p)]


class OverlapAddArgs(C.Structure):
    """ittm_overlap_add_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("offsets", C.c_void_p), ("offsets_elems", C.c_int64), ("y", C.c_void_p),
                ("y_elems", C.c_int64), ("window", C.c_void_p), ("n_rows", C.c_int), ("reserved", C.c_int), ("rows", C.POINTER(Row)),
                ("rows_dev", C.c_void_p)]


_SIGNATURES = {
    "ittm_abi_version": (C.c_int, []),
    "ittm_last_error": (C.c_char_p, []),
    "ittm_search": (C.c_int, [C.POINTER(SearchArgs), C.c_void_p]),
    "ittm_overlap_add": (C.c_int, [C.POINTER(OverlapAddArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_tempo.h declares
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
        if L.ittm_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_tempo.so ABI version mismatch")
        _lib = L
    return _lib


def table(rows):
    """(the host array of Row built from `rows` of field tuples (x_off, n, o_off, y_off, speed, 0), its bytes)."""
    arr = (Row * len(rows))(*[Row(*r) for r in rows])
    return arr, bytes(arr)


def upload(raw: bytes, device) -> torch.Tensor:
    """The bytes in a device tensor (a fresh allocation: 16-byte aligned and more)."""
    buf = bytearray(raw) + b"\0" * (16 - len(raw) % 16)         # (never empty)
    return torch.frombuffer(buf, dtype=torch.uint8).to(device)


def _check(*tensors):
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise NativeError("libindextts_tempo.so needs contiguous device tensors (no CPU fallback)")


def search(x: torch.Tensor, offsets: torch.Tensor, rows, rows_dev: int):
    """The chain of lags of every utterance `rows` names (a host array of Row; rows_dev the address of the same bytes on the
    device) of x (fp32) into offsets (int32) (ittm_search)."""
    _check(x, offsets)
    if x.dtype != torch.float32 or offsets.dtype != torch.int32:
        raise NativeError("ittm_search: x is fp32 and offsets int32")
    a = SearchArgs()
    a.x, a.x_elems, a.offsets, a.offsets_elems = _p(x), x.numel(), _p(offsets), offsets.numel()
    a.n_rows, a.rows, a.rows_dev = len(rows), rows, rows_dev
    rc = lib().ittm_search(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittm_search failed (code {rc}): {lib().ittm_last_error().decode()}")
    return offsets


def overlap_add(x: torch.Tensor, offsets: torch.Tensor, y: torch.Tensor, window: torch.Tensor, rows, rows_dev: int):
    """The outputs of every row from its samples and its lags into y (fp32) (ittm_overlap_add); window fp32 [ITTM_WIN]."""
    _check(x, offsets, y, window)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or offsets.dtype != torch.int32 or window.dtype != torch.float32 or window.numel() != WIN:
        raise NativeError(f"ittm_overlap_add: x, y and window are fp32, offsets int32, window of {WIN} elements")
    a = OverlapAddArgs()
    a.x, a.x_elems, a.offsets, a.offsets_elems = _p(x), x.numel(), _p(offsets), offsets.numel()
    a.y, a.y_elems, a.window = _p(y), y.numel(), _p(window)
    a.n_rows, a.rows, a.rows_dev = len(rows), rows, rows_dev
    rc = lib().ittm_overlap_add(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittm_overlap_add failed (code {rc}): {lib().ittm_last_error().decode()}")
    return y
