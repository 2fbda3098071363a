"""ctypes binding of libindextts_fit.so (the C ABI declared in include/indextts_fit.h): voice fitting -- the LoRA factor gradient
(ittf_lora_wgrad), the squared gradient norm (ittf_sqnorm), the AdamW step over a table of parameter segments (ittf_adamw_step) and
the ragged causal training attention, forward and backward (ittf_attn_fwd, ittf_attn_bwd).

A library of its own beside libindextts_hip.so and the eight others, loaded the same way: no CPU/PyTorch fallback -- if the shared
library is missing or a call fails, an exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from indextts._native import NativeError, _p, _stream

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_fit.so")
ABI_VERSION = 2                                     # ITTF_ABI_VERSION
CHUNK = 256                                         # ITTF_CHUNK
MAX_RANK = 64                                       # ITTF_MAX_RANK
SLICE = 4096                                        # ITTF_SLICE
ATTN_MAX_SEG = 4096                                 # ITTF_ATTN_MAX_SEG
ATTN_MAX_HEADS = 256                                # ITTF_ATTN_MAX_HEADS
ATTN_MAX_NSEG = 65535                               # ITTF_ATTN_MAX_NSEG
F32, BF16, F16 = 0, 1, 2                            # ITTF_F32, ITTF_BF16, ITTF_F16
DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


class WgradArgs(C.Structure):
    """ittf_lora_wgrad_args (include/indextts_fit.h)."""
    _fields_ = [("s", C.c_void_p), ("z", C.c_void_p), ("G", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("M", C.c_int64),
                ("r", C.c_int), ("C", C.c_int), ("lds", C.c_int), ("ldz", C.c_int), ("ldg", C.c_int), ("dtype", C.c_int),
                ("accumulate", C.c_int), ("scale", C.c_float)]


class Segment(C.Structure):
    """ittf_segment: 64 bytes."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("t_copy", C.c_void_p), ("n", C.c_int64),
                ("start", C.c_int64), ("group", C.c_int32), ("reserved", C.c_int32)]


class AdamwArgs(C.Structure):
    """ittf_adamw_args."""
    _fields_ = [("table", C.c_void_p), ("n_seg", C.c_int), ("dtype", C.c_int), ("total", C.c_int64), ("lr", C.c_double * 2),
                ("wd", C.c_double * 2), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("bc1", C.c_double),
                ("bc2_sqrt", C.c_double), ("clip", C.c_double)]


class AttnArgs(C.Structure):
    """ittf_attn_args."""
    _fields_ = [("qkv", C.c_void_p), ("out", C.c_void_p), ("lse", C.c_void_p), ("dout", C.c_void_p), ("dqkv", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("table", C.c_void_p), ("M", C.c_int64), ("n_seg", C.c_int),
                ("max_len", C.c_int), ("H", C.c_int), ("ld", C.c_int), ("ldo", C.c_int), ("scale", C.c_float)]


_SIGNATURES = {
    "ittf_abi_version": (C.c_int, []),
    "ittf_last_error": (C.c_char_p, []),
    "ittf_wgrad_ws_bytes": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "ittf_lora_wgrad": (C.c_int, [C.POINTER(WgradArgs), C.c_void_p]),
    "ittf_sqnorm_ws_floats": (C.c_int64, [C.c_int64]),
    "ittf_sqnorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ittf_adamw_step": (C.c_int, [C.POINTER(AdamwArgs), C.c_void_p]),
    "ittf_attn_ws_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "ittf_attn_fwd": (C.c_int, [C.POINTER(AttnArgs), C.c_void_p]),
    "ittf_attn_bwd": (C.c_int, [C.POINTER(AttnArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_fit.h declares
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
        if L.ittf_abi_version() != ABI_VERSION:
            raise NativeError("libindextts_fit.so ABI version mismatch")
        _lib = L
    return _lib


def _fail(who, rc):
    raise NativeError(f"{who} failed (code {rc}): {lib().ittf_last_error().decode()}")


def wgrad_ws_bytes(M: int, r: int, Cn: int) -> int:
    """The workspace ittf_lora_wgrad needs for M rows, rank r, Cn columns (host arithmetic, the header's formula)."""
    return 4 * ((M + CHUNK - 1) // CHUNK) * (16 * ((r + 15) // 16)) * Cn


def lora_wgrad(s: torch.Tensor, z: torch.Tensor, G: torch.Tensor, ws: torch.Tensor, r: int | None = None, Cn: int | None = None,
               M: int | None = None, accumulate: bool = False, scale: float = 1.0):
    """G[j, c] = (accumulate ? G : 0) + scale * sum_m s[m, j] z[m, c] for j < r, c < Cn (ittf_lora_wgrad).  s, z: 2-D device tensors
    of one type (fp32 / bf16 / fp16) whose last dimension is contiguous -- column views of a wider operand are read in place through
    their row stride; G fp32 likewise; ws: a uint8 device tensor of wgrad_ws_bytes(M, r, Cn) bytes.  r, Cn, M default to the views'
    shapes."""
    for t, name in ((s, "s"), (z, "z"), (G, "G")):
        if not (t.is_cuda and t.dim() == 2 and t.stride(1) == 1):
            raise NativeError(f"libindextts_fit.so: {name} is a 2-D device tensor with a contiguous last dimension (no CPU fallback)")
    if s.dtype not in DTYPES or z.dtype != s.dtype or G.dtype != torch.float32:
        raise NativeError("libindextts_fit.so: s and z share one of fp32 / bf16 / fp16, G is fp32")
    if not (ws.is_cuda and ws.is_contiguous() and ws.dtype == torch.uint8):
        raise NativeError("libindextts_fit.so: ws is a contiguous uint8 device tensor")
    a = WgradArgs()
    a.s, a.z, a.G, a.ws, a.ws_bytes = _p(s), _p(z), _p(G), _p(ws), ws.numel()
    a.M = s.shape[0] if M is None else int(M)
    a.r, a.C = s.shape[1] if r is None else int(r), z.shape[1] if Cn is None else int(Cn)
    if z.shape[0] < a.M or s.shape[0] < a.M or s.shape[1] < a.r or z.shape[1] < a.C or G.shape[0] < a.r or G.shape[1] < a.C:
        raise NativeError("libindextts_fit.so: s, z or G is smaller than M, r and C say")
    a.lds, a.ldz, a.ldg = s.stride(0), z.stride(0), G.stride(0)
    a.dtype, a.accumulate, a.scale = DTYPES[s.dtype], int(bool(accumulate)), float(scale)
    rc = lib().ittf_lora_wgrad(C.byref(a), _stream())
    if rc != 0:
        _fail("ittf_lora_wgrad", rc)
    return G


class SegmentTable:
    """The device table ittf_sqnorm / ittf_adamw_step walk, built from per-parameter tensors: entries (p, g, m, v, t_copy or None,
    group), all contiguous device tensors of p's element count (p, g, m, v fp32; t_copy of one dtype throughout).  Keeps the tensors
    alive, the table on the device and the squared-norm workspace."""

    def __init__(self, entries, device):
        import numpy as np
        entries = list(entries)
        if not entries:
            raise ValueError("SegmentTable: no parameter")
        recs = (Segment * len(entries))()
        start, self.dtype = 0, None
        for rec, (p, g, m, v, t, group) in zip(recs, entries):
            n = p.numel()
            for x in (p, g, m, v):
                if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.numel() == n):
                    raise NativeError("libindextts_fit.so: p, g, m and v of a segment are contiguous fp32 device tensors of one size")
            if t is not None:
                if not (t.is_cuda and t.is_contiguous() and t.dtype in DTYPES and t.numel() == n):
                    raise NativeError("libindextts_fit.so: t_copy of a segment is a contiguous device tensor of p's size")
                if self.dtype not in (None, t.dtype):
                    raise NativeError("libindextts_fit.so: every t_copy of a table has the same dtype")
                self.dtype = t.dtype
            if group not in (0, 1):
                raise ValueError("SegmentTable: group is 0 or 1")
            rec.p, rec.g, rec.m, rec.v, rec.t_copy = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if t is None else t.data_ptr()
            rec.n, rec.start, rec.group = n, start, group
            start += n
        self.entries, self.n_seg, self.total = entries, len(entries), start
        self.dtype = self.dtype or torch.float32
        self.table = torch.from_numpy(np.frombuffer(bytes(recs), dtype=np.uint8).copy()).to(device)
        self.ws = torch.empty((start + SLICE - 1) // SLICE, dtype=torch.float32, device=device)
        self.out = torch.zeros(1, dtype=torch.float32, device=device)


def sqnorm(tab: SegmentTable) -> torch.Tensor:
    """The sum of g^2 over the table's segments, fp32 [1] on the device (ittf_sqnorm)."""
    rc = lib().ittf_sqnorm(_p(tab.table), tab.n_seg, tab.total, _p(tab.ws), tab.ws.numel(), _p(tab.out), _stream())
    if rc != 0:
        _fail("ittf_sqnorm", rc)
    return tab.out


def adamw_step(tab: SegmentTable, lr, wd, t: int, clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """One AdamW step of step number t >= 1 over the table (ittf_adamw_step): lr, wd per group (pairs), clip the factor on every
    gradient.  The bias corrections 1 - beta1^t and sqrt(1 - beta2^t) are computed here in double."""
    if t < 1:
        raise ValueError("adamw_step: t counts from 1")
    a = AdamwArgs()
    a.table, a.n_seg, a.dtype, a.total = _p(tab.table), tab.n_seg, DTYPES[tab.dtype], tab.total
    a.lr[0], a.lr[1], a.wd[0], a.wd[1] = float(lr[0]), float(lr[1]), float(wd[0]), float(wd[1])
    a.beta1, a.beta2, a.eps = float(beta1), float(beta2), float(eps)
    a.bc1, a.bc2_sqrt, a.clip = 1.0 - float(beta1) ** t, (1.0 - float(beta2) ** t) ** 0.5, float(clip)
    rc = lib().ittf_adamw_step(C.byref(a), _stream())
    if rc != 0:
        _fail("ittf_adamw_step", rc)


# ------------------------------------------------------------------------------------------------------ the training attention
def attn_rows(segments, M: int):
    """The row table of ittf_attn_fwd / ittf_attn_bwd on the host: `segments` = (first row, row count) per utterance -> an int64
    array [n_seg, 2].  The kernels cannot be told a wrong table from a right one, so every refusal is here: segments in rising
    order, none overlapping the one before, all inside [0, M), each of 1 .. ATTN_MAX_SEG rows."""
    import numpy as np
    segs = [(int(f), int(n)) for f, n in segments]
    if not 1 <= len(segs) <= ATTN_MAX_NSEG:
        raise ValueError(f"attn_rows: {len(segs)} segments (1 .. {ATTN_MAX_NSEG})")
    end = 0
    for i, (f, n) in enumerate(segs):
        if not 1 <= n <= ATTN_MAX_SEG:
            raise ValueError(f"attn_rows: segment {i} has {n} rows: a segment has 1 .. {ATTN_MAX_SEG} rows (the longest the kernels take)")
        if f < 0 or f + n > int(M):
            raise ValueError(f"attn_rows: segment {i} (rows {f} .. {f + n - 1}) is out of range: the operands have {int(M)} rows")
        if i and f < segs[i - 1][0]:
            raise ValueError(f"attn_rows: segment {i} starts at row {f}, in front of segment {i - 1}: the segments come in rising order")
        if f < end:
            raise ValueError(f"attn_rows: segment {i} (first row {f}) overlaps segment {i - 1}, which ends at row {end - 1}")
        end = f + n
    return np.asarray(segs, dtype=np.int64).reshape(-1, 2)


class AttnRows:
    """attn_rows on the device: the table, n_seg, the longest segment and M.  Built once per batch."""

    def __init__(self, segments, M: int, device):
        host = attn_rows(segments, M)
        self.segments = [tuple(int(v) for v in row) for row in host]
        self.n_seg, self.max_len, self.M = int(host.shape[0]), int(host[:, 1].max()), int(M)
        self.table = torch.from_numpy(host).to(device)


def attn_ws_bytes(M: int, H: int) -> int:
    """The workspace ittf_attn_bwd needs (the header's formula)."""
    return 4 * int(M) * int(H)


def _attn_args(who, qkv, out, lse, rows: AttnRows, H, scale):
    for t, name in ((qkv, "qkv"), (out, "out")):
        if not (t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.shape[0] >= rows.M):
            raise NativeError(f"libindextts_fit.so: {who}: {name} is a 2-D fp32 device tensor of at least M rows with a contiguous last "
                              "dimension (no CPU fallback)")
    if qkv.shape[1] < 192 * H or out.shape[1] < 64 * H:
        raise NativeError(f"libindextts_fit.so: {who}: qkv has 3 * 64 H columns and out 64 H")
    if not (lse.is_cuda and lse.is_contiguous() and lse.dtype == torch.float32 and tuple(lse.shape) == (H, rows.M)):
        raise NativeError(f"libindextts_fit.so: {who}: lse is a contiguous fp32 device tensor [H, M]")
    a = AttnArgs()
    a.qkv, a.out, a.lse, a.table = _p(qkv), _p(out), _p(lse), _p(rows.table)
    a.M, a.n_seg, a.max_len, a.H, a.ld, a.ldo, a.scale = rows.M, rows.n_seg, rows.max_len, int(H), qkv.stride(0), out.stride(0), float(scale)
    return a


def attn_fwd(qkv: torch.Tensor, rows: AttnRows, H: int, scale: float = 0.125, out: torch.Tensor | None = None,
             lse: torch.Tensor | None = None):
    """Ragged causal attention over the rows of `rows` (ittf_attn_fwd): qkv fp32 [M, >= 3 * 64 H] read in place through its row
    stride -> (out fp32 [M, 64 H], lse fp32 [H, M]).  out and lse default to zero-filled tensors: rows no segment covers are not
    written."""
    M = rows.M
    out = torch.zeros(M, 64 * H, dtype=torch.float32, device=qkv.device) if out is None else out
    lse = torch.zeros(H, M, dtype=torch.float32, device=qkv.device) if lse is None else lse
    a = _attn_args("attn_fwd", qkv, out, lse, rows, H, scale)
    rc = lib().ittf_attn_fwd(C.byref(a), _stream())
    if rc != 0:
        _fail("ittf_attn_fwd", rc)
    return out, lse


def attn_bwd(qkv: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, rows: AttnRows, H: int, scale: float = 0.125,
             dqkv: torch.Tensor | None = None, ws: torch.Tensor | None = None):
    """The gradient of attn_fwd (ittf_attn_bwd) from qkv, lse and dout fp32 [M, >= 64 H] (read through its row stride) -> dqkv fp32
    with qkv's shape and row stride (zero-filled by default: uncovered rows are not written).  The forward's out is not needed.
    ws: a uint8 device tensor of attn_ws_bytes(M, H) bytes."""
    a = _attn_args("attn_bwd", qkv, dout, lse, rows, H, scale)      # (dout in out's place: the same shape rules, and ldo is its pitch)
    a.out = None
    dqkv = torch.zeros_like(qkv) if dqkv is None else dqkv
    if not (dqkv.is_cuda and dqkv.dtype == torch.float32 and dqkv.dim() == 2 and dqkv.stride(1) == 1 and dqkv.stride(0) == qkv.stride(0)
            and dqkv.shape[0] >= rows.M and dqkv.shape[1] >= 192 * H):
        raise NativeError("libindextts_fit.so: attn_bwd: dqkv is a 2-D fp32 device tensor with qkv's row stride")
    ws = torch.empty(attn_ws_bytes(rows.M, H), dtype=torch.uint8, device=qkv.device) if ws is None else ws
    if not (ws.is_cuda and ws.is_contiguous() and ws.dtype == torch.uint8):
        raise NativeError("libindextts_fit.so: ws is a contiguous uint8 device tensor")
    a.dout, a.dqkv, a.ws, a.ws_bytes = _p(dout), _p(dqkv), _p(ws), ws.numel()
    rc = lib().ittf_attn_bwd(C.byref(a), _stream())
    if rc != 0:
        _fail("ittf_attn_bwd", rc)
    return dqkv
