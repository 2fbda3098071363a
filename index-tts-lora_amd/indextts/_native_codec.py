"""ctypes binding of libindextts_codec.so (the C ABI declared in include/indextts_codec.h): the acoustic tokenizer -- the DVAE
encoder's convolutions and the nearest-code search.

A library of its own beside libindextts_hip.so, libindextts_voice.so, libindextts_audio.so, libindextts_out.so,
libindextts_post.so and libindextts_tempo.so, loaded the same way: no CPU/PyTorch fallback -- if the shared library is missing or
a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_codec.so")
ABI_VERSION = 1                                     # ITTC_ABI_VERSION
KSTEP = 32                                          # ITTC_KSTEP
CODE_RANGE = 1024                                   # ITTC_CODE_RANGE
RELU_IN, RELU_OUT, RESIDUAL = 1, 2, 4               # ITTC_RELU_IN, ITTC_RELU_OUT, ITTC_RESIDUAL


class Seg(C.Structure):
    """ittc_seg (include/indextts_codec.h)."""
    _fields_ = [("x_row0", C.c_int64), ("x_len", C.c_int64), ("y_row0", C.c_int64), ("reserved", C.c_int64)]


class ConvArgs(C.Structure):
    """ittc_conv_args."""
    _fields_ = [("x", C.c_void_p), ("x_rows", C.c_int64), ("w", C.c_void_p), ("w_elems", C.c_int64), ("bias", C.c_void_p),
                ("resid", C.c_void_p), ("y", C.c_void_p), ("y_rows", C.c_int64), ("Cin", C.c_int), ("Cout", C.c_int), ("taps", C.c_int),
                ("stride", C.c_int), ("flags", C.c_int), ("n_seg", C.c_int), ("segs", C.POINTER(Seg)), ("segs_dev", C.c_void_p)]


class NearestCodeArgs(C.Structure):
    """ittc_nearest_code_args."""
    _fields_ = [("z", C.c_void_p), ("embed", C.c_void_p), ("h", C.c_void_p), ("code", C.c_void_p), ("score", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("n_rows", C.c_int64), ("D", C.c_int), ("J", C.c_int)]


_SIGNATURES = {
    "ittc_abi_version": (C.c_int, []),
    "ittc_last_error": (C.c_char_p, []),
    "ittc_conv": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "ittc_nearest_code": (C.c_int, [C.POINTER(NearestCodeArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_codec.h declares
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
        if L.ittc_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_codec.so ABI version mismatch")
        _lib = L
    return _lib


def out_rows(x_len: int, stride: int) -> int:
    """The output rows of a clip of x_len rows (taps 1 or 3, pad (taps - 1) / 2)."""
    return (x_len + stride - 1) // stride


def packed_k(taps: int, Cin: int) -> int:
    return (taps * Cin + KSTEP - 1) // KSTEP * KSTEP


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """A conv1d weight [Cout][Cin][taps] as the packed fp32 [Kpad][Cout] of the header: W[tap Cin + c][o] = w[o][c][tap], the rows
    past taps Cin zero."""
    Cout, Cin, taps = w.shape
    out = torch.zeros(packed_k(taps, Cin), Cout, dtype=torch.float32, device=w.device)
    out[: taps * Cin] = w.to(torch.float32).permute(2, 1, 0).reshape(taps * Cin, Cout)
    return out.contiguous()


def table(segs):
    """(the host array of Seg built from `segs` of (x_row0, x_len, y_row0), its bytes)."""
    arr = (Seg * len(segs))(*[Seg(int(a), int(b), int(c), 0) for a, b, c in segs])
    return arr, bytes(arr)


def upload(raw: bytes, device) -> torch.Tensor:
    """The bytes in a device tensor (a fresh allocation: 16-byte aligned and more)."""
    buf = bytearray(raw) + b"\0" * (16 - len(raw) % 16)         # (never empty)
    return torch.frombuffer(buf, dtype=torch.uint8).to(device)


def _check(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
            raise NativeError("libindextts_codec.so needs contiguous fp32 device tensors (no CPU fallback)")


def conv(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, segs, segs_dev: int, taps: int, stride: int,
         flags: int = 0, resid: torch.Tensor | None = None):
    """y = conv(x) of every clip `segs` names (a host array of Seg; segs_dev the address of the same bytes on the device):
    x fp32 [x_rows][Cin], w the packed weights [Kpad][Cout], y fp32 [y_rows][Cout] (ittc_conv)."""
    _check(x, w, bias, y, resid)
    a = ConvArgs()
    a.x, a.x_rows, a.w, a.w_elems, a.bias = _p(x), x.shape[0], _p(w), w.numel(), _p(bias)
    a.resid = None if resid is None else _p(resid)
    a.y, a.y_rows, a.Cin, a.Cout, a.taps, a.stride, a.flags = _p(y), y.shape[0], x.shape[1], y.shape[1], taps, stride, flags
    a.n_seg, a.segs, a.segs_dev = len(segs), segs, segs_dev
    rc = lib().ittc_conv(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittc_conv failed (code {rc}): {lib().ittc_last_error().decode()}")
    return y


def ws_bytes(n_rows: int, J: int) -> int:
    """The workspace ittc_nearest_code needs for n_rows rows over J codes (0: none)."""
    n_split = (J + CODE_RANGE - 1) // CODE_RANGE
    return 8 * n_rows * n_split if n_split > 1 else 0


def nearest_code(z: torch.Tensor, embed: torch.Tensor, h: torch.Tensor, code: torch.Tensor, score: torch.Tensor | None = None,
                 ws: torch.Tensor | None = None):
    """code[r] = the nearest code of row r of z [n_rows][D] in embed [D][J] with h [J] = |e_j|^2 / 2 (ittc_nearest_code); ws: a
    uint8 device tensor of ws_bytes(n_rows, J) bytes where that is not 0."""
    _check(z, embed, h, score)
    if not code.is_cuda or code.dtype != torch.int32 or not code.is_contiguous() or code.numel() != z.shape[0] or h.numel() != embed.shape[1] \
            or embed.shape[0] != z.shape[1] or (score is not None and score.numel() != z.shape[0]):
        raise NativeError("ittc_nearest_code: code is int32 [n_rows], embed [D][J], h [J], score fp32 [n_rows]")
    a = NearestCodeArgs()
    a.z, a.embed, a.h, a.code = _p(z), _p(embed), _p(h), _p(code)
    a.score = None if score is None else _p(score)
    a.ws, a.ws_bytes = (None, 0) if ws is None else (_p(ws), ws.numel() * ws.element_size())
    a.n_rows, a.D, a.J = z.shape[0], z.shape[1], embed.shape[1]
    rc = lib().ittc_nearest_code(C.byref(a), _stream())
    if rc != 0:
        raise NativeError(f"ittc_nearest_code failed (code {rc}): {lib().ittc_last_error().decode()}")
    return code
