"""ctypes binding of libindextts_score.so (the C ABI declared in include/indextts_score.h): likelihood scoring -- the target logit
and the streamed nll / rank / lse / best of given codes under an output head.

A library of its own beside libindextts_hip.so, libindextts_voice.so, libindextts_audio.so, libindextts_out.so,
libindextts_post.so, libindextts_tempo.so and libindextts_codec.so, loaded the same way: no CPU/PyTorch fallback -- if the shared
library is missing or a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_score.so")
ABI_VERSION = 1                                     # ITTL_ABI_VERSION
RANGE = 1024                                        # ITTL_RANGE
WS_PER_ROW_RANGE = 20                               # ITTL_WS_PER_ROW_RANGE
F32, BF16, F16 = 0, 1, 2                            # ITTL_F32, ITTL_BF16, ITTL_F16
DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


class TargetLogitArgs(C.Structure):
    """ittl_target_logit_args (include/indextts_score.h)."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("n_rows", C.c_int64),
                ("D", C.c_int), ("V", C.c_int), ("ldw", C.c_int), ("dtype", C.c_int)]


class HeadNllArgs(C.Structure):
    """ittl_head_nll_args."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("nll", C.c_void_p),
                ("lse", C.c_void_p), ("best", C.c_void_p), ("rank", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("n_rows", C.c_int64), ("D", C.c_int), ("V", C.c_int), ("ldw", C.c_int), ("dtype", C.c_int)]


_SIGNATURES = {
    "ittl_abi_version": (C.c_int, []),
    "ittl_last_error": (C.c_char_p, []),
    "ittl_target_logit": (C.c_int, [C.POINTER(TargetLogitArgs), C.c_void_p]),
    "ittl_head_nll": (C.c_int, [C.POINTER(HeadNllArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_score.h declares
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
        if L.ittl_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_score.so ABI version mismatch")
        _lib = L
    return _lib


def pitch(V: int) -> int:
    """The smallest pitch of W the library takes for V columns: V rounded up to a multiple of 8."""
    return (V + 7) // 8 * 8


def ws_bytes(n_rows: int, V: int) -> int:
    """The workspace ittl_head_nll needs for n_rows rows over V columns (0: none)."""
    n_split = (V + RANGE - 1) // RANGE
    return WS_PER_ROW_RANGE * n_rows * n_split if n_split > 1 else 0


def _check(x, w, b, y, V):
    if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 2):
        raise NativeError("libindextts_score.so: x is a contiguous fp32 device tensor [n_rows][D] (no CPU fallback)")
    if not (w.is_cuda and w.is_contiguous() and w.dtype in DTYPES and w.dim() == 2 and w.shape[0] == x.shape[1]):
        raise NativeError("libindextts_score.so: w is a contiguous fp32 / bf16 / fp16 device tensor [D][ldw]")
    if not (b.is_cuda and b.is_contiguous() and b.dtype == torch.float32 and b.numel() == V):
        raise NativeError("libindextts_score.so: b is a contiguous fp32 device tensor [V]")
    if not (y.is_cuda and y.is_contiguous() and y.dtype == torch.int32 and y.numel() == x.shape[0]):
        raise NativeError("libindextts_score.so: y is a contiguous int32 device tensor [n_rows]")


def _out(t, dtype, n, name):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() == n):
        raise NativeError(f"libindextts_score.so: {name} is a contiguous {dtype} device tensor [n_rows]")
    return _p(t)


def target_logit(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, y: torch.Tensor, t: torch.Tensor, V: int | None = None):
    """t[r] = the logit of column y[r] of row r (0 where y[r] is outside [0, V)): x fp32 [n_rows][D], w [D][ldw] in fp32 / bf16 /
    fp16, b fp32 [V], y int32 [n_rows] (ittl_target_logit).  V defaults to b's length."""
    V = b.numel() if V is None else V
    _check(x, w, b, y, V)
    a = TargetLogitArgs()
    a.x, a.w, a.b, a.y, a.t = _p(x), _p(w), _p(b), _p(y), _out(t, torch.float32, x.shape[0], "t")
    a.n_rows, a.D, a.V, a.ldw, a.dtype = x.shape[0], x.shape[1], V, w.shape[1], DTYPES[w.dtype]
    rc = lib().ittl_target_logit(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittl_target_logit failed (code {rc}): {lib().ittl_last_error().decode()}")
    return t


def head_nll(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, y: torch.Tensor, t: torch.Tensor, nll: torch.Tensor, lse: torch.Tensor,
             best: torch.Tensor, rank: torch.Tensor, ws: torch.Tensor | None = None, V: int | None = None):
    """nll, lse (fp32 [n_rows]), best, rank (int32 [n_rows]) of every row from x, w, b, y and the t of target_logit
    (ittl_head_nll); ws: a uint8 device tensor of ws_bytes(n_rows, V) bytes where that is not 0."""
    V = b.numel() if V is None else V
    _check(x, w, b, y, V)
    n = x.shape[0]
    a = HeadNllArgs()
    a.x, a.w, a.b, a.y, a.t = _p(x), _p(w), _p(b), _p(y), _out(t, torch.float32, n, "t")
    a.nll, a.lse = _out(nll, torch.float32, n, "nll"), _out(lse, torch.float32, n, "lse")
    a.best, a.rank = _out(best, torch.int32, n, "best"), _out(rank, torch.int32, n, "rank")
    a.ws, a.ws_bytes = (None, 0) if ws is None else (_p(ws), ws.numel() * ws.element_size())
    a.n_rows, a.D, a.V, a.ldw, a.dtype = n, x.shape[1], V, w.shape[1], DTYPES[w.dtype]
    rc = lib().ittl_head_nll(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittl_head_nll failed (code {rc}): {lib().ittl_last_error().decode()}")
    return nll, lse, best, rank
