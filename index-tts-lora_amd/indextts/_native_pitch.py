"""ctypes binding of libindextts_pitch.so (the C ABI declared in include/indextts_pitch.h): resampling by a ratio per row, the
second step of the pitch shift.

A library of its own beside libindextts_hip.so and the other seven, loaded the same way: no CPU/PyTorch fallback -- if the shared
library is missing or a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_pitch.so")
ABI_VERSION = 1                                     # ITTR_ABI_VERSION
HW = 6                                              # ITTR_HW
PHASES = 256                                        # ITTR_PHASES
TABLE = 3076                                        # ITTR_TABLE
CUTOFF_ONE = 65536                                  # ITTR_CUTOFF_ONE
CUTOFF_MIN = 32768                                  # ITTR_CUTOFF_MIN
STEP_MIN = 1 << 31                                  # ITTR_STEP_MIN
STEP_MAX = 1 << 33                                  # ITTR_STEP_MAX
TILE = 1024                                         # ITTR_TILE


class Row(C.Structure):
    """ittr_row (include/indextts_pitch.h)."""
    _fields_ = [("x_off", C.c_int64), ("n", C.c_int64), ("y_off", C.c_int64), ("n_out", C.c_int64), ("step", C.c_uint64),
                ("cutoff", C.c_uint32), ("reserved", C.c_uint32)]


class ResampleRatioArgs(C.Structure):
    """ittr_resample_ratio_args."""
    _fields_ = [("x", C.c_void_p), ("x_elems", C.c_int64), ("y", C.c_void_p), ("y_elems", C.c_int64), ("table", C.c_void_p),
                ("n_rows", C.c_int), ("reserved", C.c_int), ("rows", C.POINTER(Row)), ("rows_dev", C.c_void_p)]


_SIGNATURES = {
    "ittr_abi_version": (C.c_int, []),
    "ittr_last_error": (C.c_char_p, []),
    "ittr_resample_ratio": (C.c_int, [C.POINTER(ResampleRatioArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_pitch.h declares
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
        if L.ittr_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_pitch.so ABI version mismatch")
        _lib = L
    return _lib


def table(rows):
    """(the host array of Row built from `rows` of field tuples (x_off, n, y_off, n_out, step, cutoff, 0), its bytes)."""
    arr = (Row * len(rows))(*[Row(*r) for r in rows])
    return arr, bytes(arr)


def resample_ratio(x: torch.Tensor, y: torch.Tensor, taps: torch.Tensor, rows, rows_dev: int):
    """The outputs of every row `rows` names (a host array of Row; rows_dev the address of the same bytes on the device) of x
    (fp32) into y (fp32) over the table `taps` (fp32 [ITTR_TABLE]) (ittr_resample_ratio)."""
    for t in (x, y, taps):
        if not t.is_cuda or not t.is_contiguous():
            raise NativeError("libindextts_pitch.so needs contiguous device tensors (no CPU fallback)")
    if x.dtype != torch.float32 or y.dtype != torch.float32 or taps.dtype != torch.float32 or taps.numel() != TABLE:
        raise NativeError(f"ittr_resample_ratio: x, y and the table are fp32, the table of {TABLE} elements")
    a = ResampleRatioArgs()
    a.x, a.x_elems, a.y, a.y_elems, a.table = _p(x), x.numel(), _p(y), y.numel(), _p(taps)
    a.n_rows, a.rows, a.rows_dev = len(rows), rows, rows_dev
    rc = lib().ittr_resample_ratio(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittr_resample_ratio failed (code {rc}): {lib().ittr_last_error().decode()}")
    return y
