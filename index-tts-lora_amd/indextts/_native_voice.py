"""ctypes binding of libindextts_voice.so (the C ABI declared in include/indextts_voice.h): the kernel of voice extraction.

A library of its own beside libindextts_hip.so, loaded the same way: no CPU/PyTorch fallback -- if the shared library is missing
or a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

F32, BF16, F16 = 0, 1, 2
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_voice.so")
ABI_VERSION = 1                                     # ITTV_ABI_VERSION
DELTA_WS_BYTES = (16 << 20) + (64 << 10)            # ITTV_DELTA_WS_BYTES


class DeltaArgs(C.Structure):
    """ittv_delta_args (include/indextts_voice.h)."""
    _fields_ = [("dtype_t", C.c_int), ("dtype_b", C.c_int), ("K", C.c_int), ("N", C.c_int), ("c", C.c_int), ("trans", C.c_int),
                ("wt", C.c_void_p), ("wb", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_int64)]


_SIGNATURES = {
    "ittv_abi_version": (C.c_int, []),
    "ittv_last_error": (C.c_char_p, []),
    "ittv_delta_project": (C.c_int, [C.POINTER(DeltaArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_voice.h declares
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
        if L.ittv_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_voice.so ABI version mismatch")
        _lib = L
    return _lib


def delta_workspace(device) -> torch.Tensor:
    """The workspace one ittv_delta_project launch at a time uses (tile counters and the slabs of a split reduction)."""
    return torch.empty(DELTA_WS_BYTES, dtype=torch.uint8, device=device)


def delta_project(wt: torch.Tensor, wb: torch.Tensor, x: torch.Tensor, trans: bool, ws: torch.Tensor, out: torch.Tensor | None = None):
    """Y = op(D) X in one launch, D = float(wt) - float(wb) formed in registers and never written (ittv_delta_project).
    wt, wb [K, N] (device; fp16, bf16 or fp32, each its own); trans False: x fp32 [N, c] -> y fp32 [K, c] = D x; trans True:
    x fp32 [K, c] -> y fp32 [N, c] = D^T x.  K and N multiples of 16, c a multiple of 16 up to 80: anything else is refused
    with a NativeError, nothing is launched.  ws: delta_workspace(device).  Same inputs, same bits."""
    for t in (wt, wb, x, ws, out):
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise NativeError("ittv_delta_project: needs contiguous device tensors (no CPU fallback)")
    if wt.dim() != 2 or wb.shape != wt.shape or wt.dtype not in _DT or wb.dtype not in _DT:
        raise NativeError(f"ittv_delta_project: wt and wb must be [K, N] alike, fp16 / bf16 / fp32 (got {tuple(wt.shape)} {wt.dtype}, "
                          f"{tuple(wb.shape)} {wb.dtype})")
    K, N = wt.shape
    rows_in, rows_out = (K, N) if trans else (N, K)
    if x.dim() != 2 or x.shape[0] != rows_in or x.dtype != torch.float32:
        raise NativeError(f"ittv_delta_project: x must be fp32 [{rows_in}, c] (got {tuple(x.shape)} {x.dtype})")
    c = int(x.shape[1])
    if out is None:
        out = torch.empty(rows_out, c, dtype=torch.float32, device=x.device)
    elif out.shape != (rows_out, c) or out.dtype != torch.float32:
        raise NativeError(f"ittv_delta_project: out must be fp32 [{rows_out}, {c}]")
    if ws.dtype != torch.uint8:
        raise NativeError("ittv_delta_project: ws must be a uint8 tensor (delta_workspace)")
    a = DeltaArgs()
    a.dtype_t, a.dtype_b = _DT[wt.dtype], _DT[wb.dtype]
    a.K, a.N, a.c, a.trans = int(K), int(N), c, int(bool(trans))
    a.wt, a.wb, a.x, a.y, a.ws, a.ws_bytes = _p(wt), _p(wb), _p(x), _p(out), _p(ws), int(ws.numel())
    rc = lib().ittv_delta_project(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittv_delta_project failed (code {rc}): {lib().ittv_last_error().decode()}")
    return out
