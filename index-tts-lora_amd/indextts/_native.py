"""ctypes binding of libindextts_hip.so (the C ABI declared in include/indextts_hip.h).

The product path has NO CPU/PyTorch fallback for the hot ops: if the shared library is missing or a call fails, an
exception is raised.  torch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

F32, BF16, F16 = 0, 1, 2
EPI_STORE, EPI_GELU_STORE, EPI_RESID_F32, EPI_QKV_CACHE, EPI_STORE_F32, EPI_SLAB_F32, EPI_SILU_STORE = 0, 1, 2, 3, 4, 5, 6
EPI_RELU_AFFINE_STORE, EPI_RELU_AFFINE_TANH_STORE = 7, 8

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libindextts_hip.so")
# tools/ only: ITTS_HIP_LIB=<.../libindextts_hip_diag.so> loads the diagnostic build (tuning overrides, time stamps) instead
_LIB_OVERRIDE = os.environ.get("ITTS_HIP_LIB")


class NativeError(RuntimeError):
    pass


class SkinnyArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("wp", C.c_void_p),
                ("bias", C.c_void_p), ("x", C.c_void_p), ("epi", C.c_int), ("y", C.c_void_p), ("yf", C.c_void_p),
                ("kcache", C.c_void_p), ("vcache", C.c_void_p), ("pos", C.c_void_p), ("heads", C.c_int),
                ("smax", C.c_int), ("ksplit", C.c_int), ("ln_c", C.c_void_p), ("ln_eps", C.c_float), ("bump", C.c_void_p),
                ("rows_per_wg", C.c_int), ("wide_wg", C.c_int), ("kv_tab", C.c_void_p), ("kv_bs", C.c_int),
                ("x_packed", C.c_int), ("y_packed", C.c_int), ("y_row0", C.c_int), ("y_mtp", C.c_int), ("x_mtp", C.c_int),
                ("post_scale", C.c_void_p), ("post_shift", C.c_void_p), ("w_scale", C.c_void_p)]


class MhaArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("Tq", C.c_int), ("Tk", C.c_int), ("H", C.c_int), ("q", C.c_void_p), ("k", C.c_void_p),
                ("v", C.c_void_p), ("q_stride", C.c_int64), ("k_stride", C.c_int64), ("v_stride", C.c_int64), ("pos", C.c_void_p),
                ("bias_u", C.c_void_p), ("bias_v", C.c_void_p), ("scale", C.c_float), ("out", C.c_void_p), ("out_mtp", C.c_int)]


class SegTableArgs(C.Structure):
    """itts_seg_table (include/indextts_hip.h)."""
    _fields_ = [("dev", C.c_void_p), ("host", C.c_void_p), ("nseg", C.c_int), ("ntiles", C.c_int)]


SEG_WORDS = 8      # ITTS_SEG_WORDS


class RowsArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("D", C.c_int), ("x", C.c_void_p), ("slab", C.c_void_p), ("nslab", C.c_int),
                ("bias", C.c_void_p), ("norm", C.c_int), ("w", C.c_void_p), ("b", C.c_void_p), ("eps", C.c_float),
                ("y", C.c_void_p), ("y_packed", C.c_void_p), ("y_row0", C.c_int), ("y_mtp", C.c_int)]


class LnReduceArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("D", C.c_int), ("h", C.c_void_p), ("slab", C.c_void_p), ("nslab", C.c_int),
                ("slab_stride", C.c_int), ("bias", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("w2", C.c_void_p),
                ("b2", C.c_void_p), ("y", C.c_void_p), ("y_packed", C.c_int), ("state_bump", C.c_void_p), ("lora_b", C.c_void_p),
                ("lora_r", C.c_int)]


class LoraShrinkArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("K", C.c_int), ("x", C.c_void_p), ("x_packed", C.c_int), ("x_mtp", C.c_int),
                ("ids", C.c_void_p), ("a_bank", C.c_void_p), ("n", C.c_int), ("rp", C.c_int), ("Kx", C.c_int), ("u", C.c_void_p),
                ("u_packed", C.c_int), ("u_mtp", C.c_int), ("ldu", C.c_int64), ("mix", C.c_void_p)]


class LoraMixEntry(C.Structure):
    _fields_ = [("id", C.c_int32), ("weight", C.c_float)]


LORA_MIX_ENTRIES = 4     # ITTS_LORA_MIX_ENTRIES
LORA_MIX_ROW_BYTES = 32


class LoraMixRow(C.Structure):
    """itts_lora_mix_row: one row's weighted mix of bank voices, 32 bytes (include/indextts_hip.h)."""
    _fields_ = [("e", LoraMixEntry * LORA_MIX_ENTRIES)]


class RefillJoinArgs(C.Structure):
    """itts_refill_join_args (include/indextts_hip.h)."""
    _fields_ = [("dtype", C.c_int), ("M", C.c_int), ("L", C.c_int), ("H", C.c_int), ("kst", C.c_void_p), ("vst", C.c_void_p),
                ("kc", C.c_void_p), ("vc", C.c_void_p), ("s_l", C.c_int64), ("s_b", C.c_int64), ("s_h", C.c_int64), ("s_p", C.c_int64),
                ("n_b", C.c_int), ("n_p", C.c_int), ("i_b", C.c_void_p), ("i_p", C.c_void_p), ("k", C.c_int), ("n_slots", C.c_int),
                ("rows", C.c_void_p), ("tok", C.c_void_p), ("fin", C.c_void_p), ("stops", C.c_void_p), ("pads", C.c_void_p),
                ("mix_new", C.c_void_p), ("step0", C.c_int), ("hist_cap", C.c_int), ("tokens", C.c_void_p), ("history", C.c_void_p),
                ("finished", C.c_void_p), ("force_stop", C.c_void_p), ("row_step0", C.c_void_p), ("pad", C.c_void_p),
                ("mix", C.c_void_p), ("state", C.c_void_p)]


class ConvArgs(C.Structure):
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("Tin", C.c_int), ("Tout", C.c_int), ("Cin", C.c_int),
                ("N", C.c_int), ("taps", C.c_int), ("off0", C.c_int), ("dil", C.c_int), ("x", C.c_void_p),
                ("x_bstride", C.c_int64), ("wp", C.c_void_p), ("bias", C.c_void_p), ("bias2", C.c_void_p),
                ("act", C.c_int), ("y", C.c_void_p), ("y_f32", C.c_int), ("y_bstride", C.c_int64),
                ("y_shift", C.c_int64), ("y_limit", C.c_int64), ("resid", C.c_void_p), ("accumulate", C.c_int),
                ("scale", C.c_float), ("valid_rows", C.c_void_p), ("ksplit", C.c_int)]


class SampleArgs(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("B", C.c_int), ("V", C.c_int), ("ldl", C.c_int), ("tokens", C.c_void_p),
                ("history", C.c_void_p), ("hist_cap", C.c_int), ("finished", C.c_void_p), ("state", C.c_void_p),
                ("extra_ids", C.c_void_p), ("n_extra", C.c_int), ("force_stop", C.c_void_p),
                ("rep_penalty", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int),
                ("do_sample", C.c_int), ("seed", C.c_uint64), ("stop_token", C.c_int), ("dbg_scores", C.c_void_p),
                ("no_advance", C.c_int), ("row_step0", C.c_void_p), ("rows", C.c_void_p)]


class SampleRow(C.Structure):
    """itts_sample_row: one row's sampling settings, 32 bytes (include/indextts_hip.h)."""
    _fields_ = [("rep_penalty", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
                ("seed", C.c_uint64), ("stream", C.c_uint32), ("do_sample", C.c_int32)]


class BeamArgs(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("B", C.c_int), ("num_beams", C.c_int), ("V", C.c_int), ("ldl", C.c_int),
                ("tokens", C.c_void_p), ("src", C.c_void_p), ("beam_scores", C.c_void_p), ("hist", C.c_void_p),
                ("hist_cap", C.c_int), ("hyp_score", C.c_void_p), ("hyp_len", C.c_void_p), ("hyp_tok", C.c_void_p),
                ("n_hyp", C.c_void_p), ("worst", C.c_void_p), ("done", C.c_void_p), ("state", C.c_void_p),
                ("extra_ids", C.c_void_p), ("n_extra", C.c_int), ("rep_penalty", C.c_float), ("temperature", C.c_float),
                ("top_p", C.c_float), ("length_penalty", C.c_float), ("top_k", C.c_int), ("do_sample", C.c_int),
                ("seed", C.c_uint64), ("eos_token", C.c_int),
                ("cand_scores", C.c_void_p), ("cand_ids", C.c_void_p), ("cand_n", C.c_void_p)]


BEAM_CAND = 1024   # ITTS_BEAM_CAND: candidate slots per row in the beam step's scratch


_SIGNATURES = {
    "itts_abi_version": (C.c_int, []),
    "itts_last_error": (C.c_char_p, []),
    "itts_last_kernel": (C.c_char_p, []),
    "itts_packed_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "itts_pack_weight": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_aa_snake_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "itts_gemm_skinny": (C.c_int, [C.POINTER(SkinnyArgs), C.c_void_p]),
    "itts_skinny_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "itts_gemm_conv": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "itts_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_ln_reduce": (C.c_int, [C.POINTER(LnReduceArgs), C.c_void_p]),
    "itts_lora_shrink": (C.c_int, [C.POINTER(LoraShrinkArgs), C.c_void_p]),
    "itts_embed_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "itts_attn_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p]),
    "itts_attn_prefill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_attn_prefill_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "itts_attn_prefill_prefix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "itts_attn_prefill_shared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p]),
    "itts_sample": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    "itts_beam_step": (C.c_int, [C.POINTER(BeamArgs), C.c_void_p]),
    "itts_beam_kv_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "itts_beam_reorder_kv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    "itts_tanh_pcm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "itts_subsample_conv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_mha_small": (C.c_int, [C.POINTER(MhaArgs), C.c_void_p]),
    "itts_glu_dwconv_ln_silu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "itts_rows": (C.c_int, [C.POINTER(RowsArgs), C.c_void_p]),
    "itts_geglu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_im2col_reflect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_res2_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_se_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_void_p]),
    "itts_scale_resid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "itts_col_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p]),
    "itts_kv_share_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "itts_prefix_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # the entry points whose per-row settings are a device table
    "itts_sample_rows": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    # the FP8 (E4M3) weight-only forms of the skinny GEMM
    "itts_packed_bytes_w8": (C.c_int64, [C.c_int, C.c_int]),
    "itts_pack_weight_w8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "itts_gemm_skinny_w8": (C.c_int, [C.POINTER(SkinnyArgs), C.c_void_p]),
    "itts_skinny_plan_w8": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    # the FP8 (E4M3) KV cache of the paged sampling loop
    "itts_attn_decode_kv8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "itts_kv8_store": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    # the sequence-mixing launches of the prompt front-end over N prompts at once
    "itts_subsample_conv_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SegTableArgs), C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p]),
    "itts_mha_small_seg": (C.c_int, [C.POINTER(MhaArgs), C.POINTER(SegTableArgs), C.c_int, C.c_void_p]),
    "itts_glu_dwconv_ln_silu_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(SegTableArgs), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    # the adapter bank's shrink launch over weighted mixes of voices
    "itts_lora_shrink_mix": (C.c_int, [C.POINTER(LoraShrinkArgs), C.c_void_p]),
    # the join of continuous batching (staged rows and their voices enter a running loop)
    "itts_refill_join": (C.c_int, [C.POINTER(RefillJoinArgs), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)          # every entry point include/indextts_hip.h declares
_lib = None


def lib():
    """Load (once) and return the shared library; raise NativeError if it is not built."""
    global _lib
    if _lib is None:
        path = _LIB_OVERRIDE or LIB_PATH
        if not os.path.exists(path):
            raise NativeError(f"{path} not found: build it with `make -C index-tts-lora_amd/csrc` "
                              f"(or python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
        L = C.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.itts_abi_version() != 10:
            raise NativeError("libindextts_hip.so ABI version mismatch")
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise NativeError(f"{what} failed (code {rc}): {lib().itts_last_error().decode()}")


def last_kernel() -> str:
    """The kernel form (with its template parameters) that this thread's last gemm_conv / aa_snake call launched, e.g.
    'conv_narrow_lds<f16,96,7,1,8,30>' or 'aa_snake_mfma<3,pair>'; '' if that call launched nothing."""
    return lib().itts_last_kernel().decode()


def dt(t: torch.dtype) -> int:
    return _DT[t]


def debug_set(key: int, value: int):
    """Tuning override of the DIAGNOSTIC build (tools/ only; include/indextts_hip_diag.h).  The product library has no
    such entry point and no mutable knobs."""
    L = lib()
    try:
        fn = L.itts_debug_set
    except AttributeError:
        raise NativeError("itts_debug_set exists only in libindextts_hip_diag.so: run the tool with "
                          "ITTS_HIP_LIB=index-tts-lora_amd/indextts/_lib/libindextts_hip_diag.so (make -C index-tts-lora_amd/csrc diag)")
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int]
    _check(fn(int(key), int(value)), "itts_debug_set")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# Held around every CUDA-graph capture and by helper threads while they enqueue work (infer.BatchPipeline): a capture in
# the default (global) error mode is invalidated by allocations / synchronisation on any other thread.
CAPTURE_LOCK = threading.RLock()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current torch stream's hipStream_t.  One of these per native launch: the raw getters (what torch's own compiled code
    paths use) cost ~0.3 us, torch.cuda.current_stream() ~8 us -- 5 ms of host time per bench step, and the prefill's ~25 us
    kernels are launched from Python at that rate."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise NativeError("HIP kernels need device tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise NativeError("HIP kernels need contiguous tensors")


# ------------------------------------------------------------------------------------------------------ wrappers
def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """w [K,N] or [taps,K,N] (device, T) -> packed uint8 buffer in MFMA B-fragment order."""
    if w.dim() == 2:
        w = w[None]
    w = w.contiguous()
    _dev(w)
    taps, K, N = w.shape
    nbytes = lib().itts_packed_bytes(taps, K, N, dt(w.dtype))
    out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _check(lib().itts_pack_weight(_p(w), _p(out), taps, K, N, dt(w.dtype), _stream()), "itts_pack_weight")
    return out


def aa_snake(x, alpha_log, beta_log, up_f, down_f, layout=0, out=None, valid_rows=None):
    """x [B,T,C] (layout 0) or [B,C,T] (layout 1); filters are HOST float32 tensors/arrays of 12 taps.
    valid_rows int32 [B] (layout 0): per-element sequence lengths of a ragged batch (rows past them are not written)."""
    _dev(x, alpha_log, beta_log)
    if layout == 0:
        B, T, Cn = x.shape
    else:
        B, Cn, T = x.shape
    y = torch.empty_like(x) if out is None else out
    uf = (C.c_float * 12)(*[float(v) for v in up_f])
    df = (C.c_float * 12)(*[float(v) for v in down_f])
    _check(lib().itts_aa_snake_fwd(_p(x), _p(y), _p(alpha_log), _p(beta_log), C.cast(uf, C.c_void_p),
                                   C.cast(df, C.c_void_p), B, T, Cn, dt(x.dtype), layout, _p(valid_rows), _stream()),
           "itts_aa_snake_fwd")
    return y


def gemm_skinny(dtype, M, N, K, wp, bias=None, x=None, epi=EPI_STORE, y=None, yf=None, kcache=None, vcache=None, pos=None,
                heads=0, smax=0, ksplit=1, x_packed=False, y_packed=False, ln_c=None, ln_eps=1e-5, bump=None, rows_per_wg=0,
                wide_wg=False, kv_tab=None, kv_bs=0, y_row0=0, y_mtp=0, x_mtp=0, post=None, w_scale=None):
    """ln_c fp32 [N]: LayerNorm folded into the GEMM -- x holds the RAW rows, wp = pack(gamma . W), bias = beta W + b
    (see itts_skinny_args).  EPI_RESID_F32: yf += x W + bias, and y (optional, T) receives a copy of the new rows.
    bump: int32 device word the launch increments.  rows_per_wg / wide_wg: launch-geometry hints.
    y_row0 / y_mtp: a packed y's rows land at [y_row0, y_row0 + M) of an operand of y_mtp row tiles; x_mtp: a packed x is the
    first M rows of an operand of x_mtp row tiles.  post = (scale, shift) fp32 [N]: the EPI_RELU_AFFINE_* epilogues.
    w_scale fp32 [N]: wp = pack_weight_w8(codes), FP8 weights -- the launch goes to itts_gemm_skinny_w8 (see gemm_skinny_w8)."""
    a = SkinnyArgs()
    a.dtype, a.M, a.N, a.K = dt(dtype), M, N, K
    a.wp, a.bias, a.x = _p(wp), _p(bias), _p(x)
    a.epi, a.y, a.yf = epi, _p(y), _p(yf)
    a.kcache, a.vcache, a.pos, a.heads, a.smax, a.ksplit = _p(kcache), _p(vcache), _p(pos), heads, smax, ksplit
    a.x_packed, a.y_packed = int(bool(x_packed)), int(bool(y_packed))
    a.ln_c, a.ln_eps, a.bump = _p(ln_c), float(ln_eps), _p(bump)
    a.rows_per_wg, a.wide_wg = int(rows_per_wg), int(bool(wide_wg))
    a.kv_tab, a.kv_bs = _p(kv_tab), int(kv_bs)
    a.y_row0, a.y_mtp, a.x_mtp = int(y_row0), int(y_mtp), int(x_mtp)
    if post is not None:
        a.post_scale, a.post_shift = _p(post[0]), _p(post[1])
    if w_scale is None:
        _check(lib().itts_gemm_skinny(C.byref(a), _stream()), "itts_gemm_skinny")
    else:
        a.w_scale = _p(w_scale)
        _check(lib().itts_gemm_skinny_w8(C.byref(a), _stream()), "itts_gemm_skinny_w8")


def pack_weight_w8(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [K, N] (device; E4M3 codes of utils/quant.quantize_e4m3_cols) -> the packed FP8 weight image
    (include/indextts_hip.h: 1-KiB blocks of 16 columns x 64 k)."""
    codes = codes.contiguous()
    _dev(codes)
    if codes.dtype != torch.uint8 or codes.dim() != 2:
        raise NativeError("itts_pack_weight_w8: codes must be uint8 [K, N]")
    K, N = codes.shape
    out = torch.empty(lib().itts_packed_bytes_w8(K, N), dtype=torch.uint8, device=codes.device)
    _check(lib().itts_pack_weight_w8(_p(codes), _p(out), K, N, _stream()), "itts_pack_weight_w8")
    return out


def gemm_skinny_w8(dtype, M, N, K, wp, w_scale, *args, **kw):
    """gemm_skinny over FP8 weights: wp = pack_weight_w8(codes), w_scale fp32 [N]; the accumulator is scaled per column in front
    of the epilogue.  dtype: the activation type (bf16 / f16).  ln_c = w_scale * column sums of the decoded codes (folded form).
    The other arguments are gemm_skinny's (wide_wg is ignored: there is no 16-wave FP8 form)."""
    if w_scale is None:
        raise NativeError("itts_gemm_skinny_w8 failed (code 1): itts_gemm_skinny_w8: w_scale is null")
    gemm_skinny(dtype, M, N, K, wp, *args, w_scale=w_scale, **kw)


def _plan_dict(out) -> dict:
    return dict(grid=(out[0], out[1], out[6]), waves=out[2], tiles_per_wg=out[3], ksteps_per_wave=out[4], lds=out[5],
                row_tiles_per_wg=out[7])


def skinny_plan_w8(dtype, M, N, K, rows_per_wg=0, fold=False) -> dict:
    """Launch geometry itts_gemm_skinny_w8 would use (host-only); ksteps_per_wave counts 64-k weight blocks."""
    out = (C.c_int * 8)()
    _check(lib().itts_skinny_plan_w8(dt(dtype), M, N, K, int(rows_per_wg), int(bool(fold)), out), "itts_skinny_plan_w8")
    return _plan_dict(out)


def subsample_conv(mel, w, b, y):
    """mel fp32 [T, F], w fp32 [C, 9], b [C] -> y T [T2, C * F2] = relu(conv2d 3x3 stride 2), laid out for the Linear behind it."""
    _dev(mel, w, b, y)
    T, Fq = mel.shape
    _check(lib().itts_subsample_conv(_p(mel), _p(w), _p(b), _p(y), T, Fq, w.shape[0], dt(y.dtype), _stream()), "itts_subsample_conv")
    return y


def _mha_args(q, k, v, out, Tq, Tk, H, q_stride, k_stride, v_stride, out_mtp, scale, pos, bias_u, bias_v):
    a = MhaArgs()
    a.dtype, a.Tq, a.Tk, a.H = dt(out.dtype), Tq, Tk, H
    a.q, a.k, a.v = _p(q), _p(k), _p(v)
    a.q_stride, a.k_stride, a.v_stride = q_stride, k_stride, v_stride
    a.pos, a.bias_u, a.bias_v = _p(pos), _p(bias_u), _p(bias_v)
    a.scale, a.out, a.out_mtp = float(scale), _p(out), int(out_mtp)
    return a


def mha_small(q, k, v, out, Tq, Tk, H, q_stride, k_stride, v_stride, out_mtp, scale, pos=None, bias_u=None, bias_v=None):
    """Short-sequence attention (head dim 64) into the packed layout; pos / bias_u / bias_v: the Conformer's relative-position term.
    q / k / v may be views into one buffer (pointer + row stride in elements)."""
    a = _mha_args(q, k, v, out, Tq, Tk, H, q_stride, k_stride, v_stride, out_mtp, scale, pos, bias_u, bias_v)
    _check(lib().itts_mha_small(C.byref(a), _stream()), "itts_mha_small")
    return out


def glu_dwconv_ln_silu(x, w, b, ln_w, ln_b, y, T, Cn, y_mtp, eps=1e-5):
    """x T [T, 2C] -> GLU -> depthwise conv (w fp32 [C, taps]) -> LayerNorm -> SiLU -> y T packed [T, C]."""
    _dev(x, w, b, ln_w, ln_b, y)
    _check(lib().itts_glu_dwconv_ln_silu(_p(x), _p(w), _p(b), _p(ln_w), _p(ln_b), _p(y), T, Cn, w.shape[1], int(y_mtp), float(eps),
                                         dt(y.dtype), _stream()), "itts_glu_dwconv_ln_silu")
    return y


def seg_words(records, ntiles, tile_map=None) -> torch.Tensor:
    """The words of a segment table (include/indextts_hip.h) as a host int32 tensor: one record of up to SEG_WORDS ints
    per segment (row0, len, ...; missing words are 0), then the segment of every 16-row tile of the row space (-1: none).
    tile_map: given instead of derived (the derived map names, per tile, the last segment whose rows touch it)."""
    recs = [list(map(int, r)) + [0] * (SEG_WORDS - len(r)) for r in records]
    if not recs or any(len(r) != SEG_WORDS for r in recs):
        raise ValueError(f"a segment table takes at least one record of at most {SEG_WORDS} words")
    if tile_map is None:
        tile_map = [-1] * int(ntiles)
        for s, r in enumerate(recs):
            for tile in range(max(r[0], 0) // 16, min((r[0] + max(r[1], 0) + 15) // 16, int(ntiles))):
                tile_map[tile] = s
    if len(tile_map) != int(ntiles):
        raise ValueError("the tile map has one entry per row tile")
    return torch.tensor([w for r in recs for w in r] + [int(v) for v in tile_map], dtype=torch.int32)


class SegTable:
    """A segment table on the host and on `device`, with the itts_seg_table that names both (the tensors live as long as this)."""

    def __init__(self, records, ntiles, device, tile_map=None):
        self.host = seg_words(records, ntiles, tile_map)
        self.dev = self.host.to(device)
        self.nseg, self.ntiles = len(records), int(ntiles)
        self.args = SegTableArgs(C.c_void_p(self.dev.data_ptr()), C.c_void_p(self.host.data_ptr()), self.nseg, self.ntiles)


def subsample_conv_seg(mel, w, b, y, tab: SegTable):
    """subsample_conv over the prompts whose frames follow one another in mel fp32 [frames, F]; y T [ntiles * 16, C * F2]."""
    _dev(mel, w, b, y)
    frames, Fq = mel.shape
    _check(lib().itts_subsample_conv_seg(_p(mel), _p(w), _p(b), _p(y), C.byref(tab.args), frames, Fq, w.shape[0], dt(y.dtype), _stream()),
           "itts_subsample_conv_seg")
    return y


def mha_small_seg(q, k, v, out, q_rows, kv_rows, H, q_stride, k_stride, v_stride, out_mtp, scale, tab: SegTable, pos=None, bias_u=None,
                  bias_v=None, pos_tk=0):
    """mha_small over the segments of `tab`: q / k / v point at row 0 of their row spaces of q_rows / kv_rows rows; pos T
    [H, pos_tk, 64] is indexed by the key's index within its segment."""
    a = _mha_args(q, k, v, out, q_rows, kv_rows, H, q_stride, k_stride, v_stride, out_mtp, scale, pos, bias_u, bias_v)
    _check(lib().itts_mha_small_seg(C.byref(a), C.byref(tab.args), int(pos_tk), _stream()), "itts_mha_small_seg")
    return out


def glu_dwconv_ln_silu_seg(x, w, b, ln_w, ln_b, y, Cn, y_mtp, tab: SegTable, eps=1e-5):
    """glu_dwconv_ln_silu over the segments of `tab`: x T [ntiles * 16, 2C] -> y T packed, y_mtp >= ntiles row tiles."""
    _dev(x, w, b, ln_w, ln_b, y)
    _check(lib().itts_glu_dwconv_ln_silu_seg(_p(x), _p(w), _p(b), _p(ln_w), _p(ln_b), _p(y), C.byref(tab.args), Cn, w.shape[1],
                                             int(y_mtp), float(eps), dt(y.dtype), _stream()), "itts_glu_dwconv_ln_silu_seg")
    return y


def rows(M, D, dtype, x=None, slab=None, nslab=0, bias=None, norm=0, w=None, b=None, eps=1e-5, y=None, y_packed=None, y_row0=0,
         y_mtp=0):
    """Row operations on an fp32 stream: (x) + bias + sum(slabs) -> [LayerNorm | l2-normalise * sqrt(D) * w] -> y fp32 and / or a
    packed T copy (itts_rows)."""
    a = RowsArgs()
    a.dtype, a.M, a.D = dt(dtype), M, D
    a.x, a.slab, a.nslab, a.bias = _p(x), _p(slab), int(nslab), _p(bias)
    a.norm, a.w, a.b, a.eps = int(norm), _p(w), _p(b), float(eps)
    a.y, a.y_packed, a.y_row0, a.y_mtp = _p(y), _p(y_packed), int(y_row0), int(y_mtp)
    _check(lib().itts_rows(C.byref(a), _stream()), "itts_rows")


def geglu(h, y, M, Kp, y_mtp=0):
    """h T [M, 2 Kp] (x | gate) -> y T packed [M, Kp] = gelu(gate) * x."""
    _dev(h, y)
    _check(lib().itts_geglu(_p(h), _p(y), M, Kp, int(y_mtp), dt(y.dtype), _stream()), "itts_geglu")
    return y


def prefix_rows(text, conds, text_emb, text_pos, start_tok, stop_tok):
    """text int64 [B, L], conds fp32 [1 | B, C, D] -> (emb fp32 [B, P, D], mask int64 [B, P + 1], pad int32 [B]), P = C + L + 2:
    the GPT prompt rows of prepare_gpt_inputs in one launch (itts_prefix_rows)."""
    _dev(text, conds, text_emb, text_pos)
    B, L = text.shape
    Bc, Cn, D = conds.shape
    P = Cn + L + 2
    emb = torch.empty(B, P, D, dtype=torch.float32, device=text.device)
    mask = torch.empty(B, P + 1, dtype=torch.int64, device=text.device)
    pad = torch.empty(B, dtype=torch.int32, device=text.device)
    _check(lib().itts_prefix_rows(_p(text), _p(conds), Bc, _p(text_emb), _p(text_pos), _p(emb), _p(mask), _p(pad), B, L, Cn, D,
                                  int(start_tok), int(stop_tok), text_emb.shape[0], text_pos.shape[0], _stream()), "itts_prefix_rows")
    return emb, mask, pad


def im2col_reflect(x, y, taps, dil, Kp, y_mtp):
    """x fp32 [T, F] -> y T packed [T, Kp]: the k-tap reflect-padded convolution's operand (itts_im2col_reflect)."""
    _dev(x, y)
    _check(lib().itts_im2col_reflect(_p(x), _p(y), x.shape[0], x.shape[1], taps, dil, Kp, y_mtp, dt(y.dtype), _stream()), "itts_im2col_reflect")


def res2_step(y1, cat, wp, bias, scale, shift, T, mtp, chunk, dil, first):
    _check(lib().itts_res2_step(_p(y1), _p(cat), _p(wp), _p(bias), _p(scale), _p(shift), T, mtp, chunk, dil, int(bool(first)),
                                dt(cat.dtype), _stream()), "itts_res2_step")


def se_gate(y, w1, b1, w2, b2, gate, T, Cn, H, mtp):
    _dev(y, w1, b1, w2, b2, gate)
    _check(lib().itts_se_gate(_p(y), _p(w1), _p(b1), _p(w2), _p(b2), _p(gate), T, Cn, H, mtp, dt(y.dtype), _stream()), "itts_se_gate")


def scale_resid(y, res, gate, out, T, Cn, mtp):
    """out = gate * y + res over packed [T, Cn] operands (res / out may be k-step runs of a wider packed operand: views)."""
    _check(lib().itts_scale_resid(_p(y), _p(res), _p(gate), _p(out), T, Cn, mtp, dt(y.dtype), _stream()), "itts_scale_resid")


def col_stats(x, out, T, Cn, mtp, logit=None, scale=None, shift=None):
    """out T [2 Cn] = [mean | std] over time of packed x [T, Cn], optionally softmax(logit)-weighted and affine-mapped."""
    _check(lib().itts_col_stats(_p(x), _p(logit), _p(scale), _p(shift), _p(out), T, Cn, mtp, dt(out.dtype), _stream()), "itts_col_stats")


def packed_rows(M: int) -> int:
    """Rows a packed-activation buffer must provide for M logical rows (16-row tiles)."""
    return (M + 15) // 16 * 16


def pack_activation(x: torch.Tensor) -> torch.Tensor:
    """Row-major [M, K] -> the packed activation layout (include/indextts_hip.h), as a flat tensor of packed_rows(M)*K
    elements.  Host-side torch restatement for tests and tools; the kernels write this layout themselves."""
    M, K = x.shape
    E = 4 if x.dtype == torch.float32 else 8
    KS = 4 * E
    mtp = (M + 15) // 16
    xp = torch.zeros(mtp * 16, K, dtype=x.dtype, device=x.device)
    xp[:M] = x
    v = xp.view(mtp, 16, K // KS, 4, E).permute(2, 0, 3, 1, 4).contiguous()   # [ks][mt][g][c][e]
    return v.view(-1)


def unpack_activation(xp: torch.Tensor, M: int, K: int) -> torch.Tensor:
    E = 4 if xp.dtype == torch.float32 else 8
    KS = 4 * E
    mtp = (M + 15) // 16
    v = xp.view(K // KS, mtp, 4, 16, E).permute(1, 3, 0, 2, 4).contiguous().view(mtp * 16, K)
    return v[:M]


def skinny_plan(dtype, M, N, K, ksplit=1, rows_per_wg=0, wide_wg=False, fold=False) -> dict:
    """Launch geometry itts_gemm_skinny would use (host-only)."""
    out = (C.c_int * 8)()
    _check(lib().itts_skinny_plan(dt(dtype), M, N, K, ksplit, int(rows_per_wg), int(bool(wide_wg)), int(bool(fold)), out),
           "itts_skinny_plan")
    return _plan_dict(out)


def gemm_conv(dtype, B, Tin, Tout, Cin, N, wp, x, y, taps=1, off0=0, dil=1, x_bstride=None, bias=None, bias2=None,
              act=0, y_f32=False, y_bstride=None, y_shift=0, y_limit=None, resid=None, accumulate=False, scale=1.0,
              valid_rows=None, ksplit=1):
    """valid_rows int32 [B]: ragged batch -- input rows >= valid_rows[b] read as zeros, tiles that only see them are skipped."""
    a = ConvArgs()
    a.dtype, a.B, a.Tin, a.Tout, a.Cin, a.N = dt(dtype), B, Tin, Tout, Cin, N
    a.taps, a.off0, a.dil = taps, off0, dil
    a.x, a.x_bstride = _p(x), Tin * Cin if x_bstride is None else x_bstride
    a.wp, a.bias, a.bias2, a.act = _p(wp), _p(bias), _p(bias2), act
    a.y, a.y_f32 = _p(y), int(y_f32)
    a.y_bstride = Tout * N if y_bstride is None else y_bstride
    a.y_shift = y_shift
    a.y_limit = Tout * N if y_limit is None else y_limit
    a.resid, a.accumulate, a.scale = _p(resid), int(accumulate), float(scale)
    a.valid_rows = _p(valid_rows)
    a.ksplit = int(ksplit)
    _check(lib().itts_gemm_conv(C.byref(a), _stream()), "itts_gemm_conv")


def layernorm(h, w, b, out, w2=None, b2=None):
    """h fp32 [M,D] -> out (T or fp32) [M,D]."""
    _dev(h, w, b, out)
    M, D = h.shape
    y_f32 = out.dtype == torch.float32
    d = F32 if y_f32 else dt(out.dtype)
    _check(lib().itts_layernorm(_p(h), _p(w), _p(b), _p(w2), _p(b2), _p(out), int(y_f32), M, D, d, _stream()),
           "itts_layernorm")
    return out


def ln_reduce(h, w, b, out, slab=None, nslab=0, bias=None, w2=None, b2=None, state_bump=None, y_packed=False, slab_stride=0,
              lora_b=None):
    """h fp32 [M,D] (updated in place when nslab > 0) -> out T [M,D] = LN(h + bias + sum(slabs) [+ (x A) lora_b]).
    state_bump: int32[2] device words incremented once by the launch (decode loop: step counter and cache position).
    lora_b fp32 [r, D] (= B^T alpha/r-free: the scale rides on A): runtime LoRA of the producing projection, whose slabs are
    slab_stride = D + 16*ceil(r/16) wide."""
    M, D = h.shape
    a = LnReduceArgs()
    a.dtype, a.M, a.D = dt(out.dtype), M, D
    a.h, a.slab, a.nslab, a.slab_stride = _p(h), _p(slab), int(nslab), int(slab_stride)
    a.bias, a.w, a.b, a.w2, a.b2 = _p(bias), _p(w), _p(b), _p(w2), _p(b2)
    a.y, a.y_packed, a.state_bump = _p(out), int(bool(y_packed)), _p(state_bump)
    if lora_b is not None:
        a.lora_b, a.lora_r = _p(lora_b), lora_b.shape[0]
    _check(lib().itts_ln_reduce(C.byref(a), _stream()), "itts_ln_reduce")
    return out


def lora_kx(n: int, rp: int) -> int:
    """Operand columns a bank of n adapters of padded rank rp adds to a GEMM: n * rp rounded up to whole k-steps of either type."""
    return (n * rp + 31) // 32 * 32


def lora_shrink(x, ids, a_bank, u, M, K, x_packed=False, x_mtp=0, u_packed=False, u_mtp=0, ldu=0, mix=None):
    """The shrink half of the per-row LoRA adapter bank (itts_lora_shrink): u[m][ids[m] * rp + j] = x[m] . a_bank[ids[m]][j], every
    other column of u[m][:Kx] zero.  x T [M, K] (row-major or packed), ids int32 [M] on the device (-1 = no adapter), a_bank T
    [n, rp, K]; u: the packed operand's tail (u_packed: a tensor that starts at the first appended block) or row-major with the
    leading dimension ldu (a view that starts at the row's first extra column).
    mix (instead of ids, which is then None): the launch over weighted mixes, itts_lora_shrink_mix (see lora_shrink_mix)."""
    if (ids is None) == (mix is None):
        raise ValueError("lora_shrink takes ids or mix, one of them")
    if mix is None:
        who, fn = "itts_lora_shrink", lib().itts_lora_shrink
        _dev(ids, a_bank)
        if ids.dtype != torch.int32 or ids.numel() < M:
            raise NativeError("itts_lora_shrink: ids must be int32 [M]")
    else:
        who, fn = "itts_lora_shrink_mix", lib().itts_lora_shrink_mix
        _dev(mix, a_bank)
        if mix.dtype != torch.uint8 or mix.numel() < M * LORA_MIX_ROW_BYTES:
            raise NativeError("itts_lora_shrink_mix: mix must be a uint8 device tensor of M 32-byte records")
    n, rp, Ka = a_bank.shape
    if Ka != K or a_bank.dtype != x.dtype or u.dtype != x.dtype:
        raise NativeError(f"{who}: a_bank must be T [n, rp, K] of the operand's type")
    a = LoraShrinkArgs()
    a.dtype, a.M, a.K = dt(x.dtype), int(M), int(K)
    a.x, a.x_packed, a.x_mtp = _p(x), int(bool(x_packed)), int(x_mtp)
    a.ids, a.mix, a.a_bank, a.n, a.rp, a.Kx = _p(ids), _p(mix), _p(a_bank), n, rp, lora_kx(n, rp)
    a.u, a.u_packed, a.u_mtp, a.ldu = _p(u), int(bool(u_packed)), int(u_mtp), int(ldu)
    _check(fn(C.byref(a), _stream()), who)


def pack_lora_mix(mixes):
    """Normalised mixes (one tuple of up to four (id, weight) per row: GPTEngine.check_adapter_mix) -> numpy uint8 [len(mixes), 32]:
    the records itts_lora_shrink_mix reads (itts_lora_mix_row; unused entries are id -1, weight 0)."""
    import numpy as np
    recs = (LoraMixRow * max(len(mixes), 1))()
    for rec, mix in zip(recs, mixes):
        if len(mix) > LORA_MIX_ENTRIES:
            raise ValueError(f"a mix holds at most {LORA_MIX_ENTRIES} entries (got {len(mix)})")
        for j in range(LORA_MIX_ENTRIES):
            rec.e[j].id, rec.e[j].weight = (int(mix[j][0]), float(mix[j][1])) if j < len(mix) else (-1, 0.0)
    return np.frombuffer(bytes(recs), dtype=np.uint8).reshape(-1, LORA_MIX_ROW_BYTES)[: len(mixes)].copy()


def refill_join(kst, vst, kc, vc, i_b, i_p, rows, tok, fin, stops, pads, step0, tokens, history, finished, force_stop, row_step0,
                pad, state, mix_new=None, mix=None):
    """The join of continuous batching in one launch (itts_refill_join).  kst / vst T [M, L, H, 64]: the staged keys / values of M
    positions; they go to (i_b[m], i_p[m]) of the caches kc / vc, T [L, n_b, H, n_p, 64] -- the paged pool (block, offset) or the
    contiguous rows (cache row, position); i_b / i_p int32 [M].  rows int32 [k]: the slots the k new rows take; tok / fin / stops /
    pads int32 [k] and mix_new uint8 [k, 32] are written to tokens / history[:, 0] / finished / force_stop / pad / mix of those slots,
    row_step0 of those slots <- step0, and state[2] -= k.  An i_b, i_p or slot outside its table is skipped."""
    _dev(kst, vst, kc, vc, i_b, i_p, rows, tok, fin, stops, pads, tokens, history, finished, force_stop, row_step0, pad, state, mix_new, mix)
    M, L, H = int(kst.shape[0]), int(kc.shape[0]), int(kc.shape[2])
    k = int(rows.numel())
    if kc.dim() != 5 or kc.shape[4] != 64 or kc.shape != vc.shape or kc.dtype != vc.dtype or kc.dtype not in _DT:
        raise NativeError("itts_refill_join: the caches must be T [L, n_b, H, n_p, 64], K and V alike")
    if kst.shape != (M, L, H, 64) or vst.shape != kst.shape or kst.dtype != kc.dtype or vst.dtype != kc.dtype:
        raise NativeError("itts_refill_join: kst / vst must be [M, L, H, 64] of the cache's type")
    ints = (i_b, i_p, rows, tok, fin, stops, pads, tokens, history, finished, force_stop, row_step0, pad, state)
    if any(t.dtype != torch.int32 for t in ints) or i_b.numel() != M or i_p.numel() != M:
        raise NativeError("itts_refill_join: indices and row state must be int32 (i_b, i_p: [M])")
    if any(t.numel() != k for t in (tok, fin, stops, pads)) or state.numel() < 3 or history.dim() != 2:
        raise NativeError("itts_refill_join: tok, fin, stops and pads hold one entry per entering row; history is [slots, cap]")
    n_slots = min(int(t.shape[0]) for t in (tokens, history, finished, force_stop, row_step0, pad))
    if (mix is None) != (mix_new is None):
        raise NativeError("itts_refill_join: mix and mix_new go together")
    if mix is not None:
        if mix.dtype != torch.uint8 or mix_new.dtype != torch.uint8 or mix_new.numel() != k * LORA_MIX_ROW_BYTES or \
                mix.numel() % LORA_MIX_ROW_BYTES:
            raise NativeError("itts_refill_join: mix / mix_new must be uint8 tables of 32-byte records (mix_new: k of them)")
        n_slots = min(n_slots, mix.numel() // LORA_MIX_ROW_BYTES)
    a = RefillJoinArgs()
    a.dtype, a.M, a.L, a.H = dt(kc.dtype), M, L, H
    a.kst, a.vst, a.kc, a.vc = _p(kst), _p(vst), _p(kc), _p(vc)
    a.s_l, a.s_b, a.s_h, a.s_p = (int(v) for v in kc.stride()[:4])
    a.n_b, a.n_p, a.i_b, a.i_p = int(kc.shape[1]), int(kc.shape[3]), _p(i_b), _p(i_p)
    a.k, a.n_slots, a.rows, a.tok, a.fin, a.stops, a.pads, a.mix_new = k, n_slots, _p(rows), _p(tok), _p(fin), _p(stops), _p(pads), _p(mix_new)
    a.step0, a.hist_cap = int(step0), int(history.shape[1])
    a.tokens, a.history, a.finished, a.force_stop, a.row_step0, a.pad = (_p(t) for t in (tokens, history, finished, force_stop, row_step0, pad))
    a.mix, a.state = _p(mix), _p(state)
    _check(lib().itts_refill_join(C.byref(a), _stream()), "itts_refill_join")


def lora_shrink_mix(x, mix, a_bank, u, M, K, **kw):
    """lora_shrink over weighted mixes (itts_lora_shrink_mix): for every entry (a, w) of row m's record u[m][a * rp + j] =
    w * (x[m] . a_bank[a][j]), every other column of u[m][:Kx] zero.  mix: uint8 device tensor [>= M, 32] of packed records
    (pack_lora_mix; the values are checked on the host before the upload, the kernel only guards memory); the other arguments are
    lora_shrink's."""
    lora_shrink(x, None, a_bank, u, M, K, mix=mix, **kw)


def embed_step(tokens, table, pos_table, step, pos_add, h, bump=None, row_step0=None, h_packed=None):
    """bump (int32 device word or None) is incremented once (the decode loop's cache position).
    row_step0 (int32 [B] or None): the loop step at which each row started (slot refill).
    h_packed (T, packed activation layout, or None): T-typed copy of the rows for the LayerNorm-folded QKV GEMM."""
    B, D = h.shape
    d = F32 if h_packed is None else dt(h_packed.dtype)
    _check(lib().itts_embed_step(_p(tokens), _p(table), _p(pos_table), _p(step), pos_add, _p(h), B, D, _p(bump), _p(row_step0),
                                 pos_table.shape[0], _p(h_packed), d, _stream()), "itts_embed_step")


def attn_decode(q, kcache, vcache, out, pad, pos, B, H, smax, out_packed=False, kv_rows=None, kv_step=None, skip_rows=None,
                kv_share=None, kv_tab=None, kv_bs=0):
    """kv_rows int32 [2][B][smax] + kv_step (device word): beam-search row table instead of permuted cache rows.
    skip_rows int32 [B]: rows with a nonzero entry are left out (their slice of `out` is not written).
    kv_share (device word (p0 << 8) | C): the first C keys of every row equal cache row 0's positions [p0, p0 + C)."""
    _check(lib().itts_attn_decode(_p(q), _p(kcache), _p(vcache), _p(out), _p(pad), _p(pos), B, H, smax, dt(q.dtype),
                                  int(bool(out_packed)), _p(kv_rows), _p(kv_step), _p(skip_rows), _p(kv_share), _p(kv_tab), int(kv_bs),
                                  _stream()),
           "itts_attn_decode")


def attn_decode_kv8(qkv, kcache, vcache, out, pad, pos, kv_scale, B, H, out_packed=False, skip_rows=None, kv_tab=None, kv_bs=0):
    """The decode step's attention over an FP8 paged cache, with the append of the step's own key / value
    (include/indextts_hip.h).  qkv T [B][3 * H * 64]; kcache / vcache uint8 pools of one layer; kv_scale fp32 [2][H]."""
    _check(lib().itts_attn_decode_kv8(_p(qkv), _p(kcache), _p(vcache), _p(out), _p(pad), _p(pos), _p(kv_scale), B, H, dt(qkv.dtype),
                                      int(bool(out_packed)), _p(skip_rows), _p(kv_tab), int(kv_bs), _stream()), "itts_attn_decode_kv8")


def kv8_store(qkv, kcache, vcache, kv_scale, B, S, H, pad=None, row_off=None, cache_shift=None, kv_tab=None, kv_bs=0):
    """The prefill's k / v thirds of qkv T [rows][3 * H * 64] -> E4M3 codes in the paged pool of one layer
    (include/indextts_hip.h): rows [B][S] with pad, or packed rows with row_off / cache_shift."""
    _dev(qkv, kcache, vcache, kv_scale)
    _check(lib().itts_kv8_store(_p(qkv), _p(kcache), _p(vcache), _p(kv_scale), _p(pad), _p(row_off), _p(cache_shift), B, S, H,
                                dt(qkv.dtype), _p(kv_tab), int(kv_bs), _stream()), "itts_kv8_store")


def attn_prefill(qkv, out, kcache, vcache, pad, B, S, H, smax):
    _check(lib().itts_attn_prefill(_p(qkv), _p(out), _p(kcache), _p(vcache), _p(pad), B, S, H, smax, dt(qkv.dtype),
                                   _stream()), "itts_attn_prefill")


def attn_prefill_packed(qkv, out, kcache, vcache, row_off, cache_shift, B, Smax, H, smax, kv_tab=None, kv_bs=0):
    """Packed rows (no padding): row_off int32 [B+1]; cache row of local row i = cache_shift[b] + i.
    kv_tab / kv_bs: the caches are a paged pool behind a block table (include/indextts_hip.h)."""
    _check(lib().itts_attn_prefill_packed(_p(qkv), _p(out), _p(kcache), _p(vcache), _p(row_off), _p(cache_shift), B, Smax, H,
                                          smax, dt(qkv.dtype), _p(kv_tab), int(kv_bs), _stream()), "itts_attn_prefill_packed")


def attn_prefill_prefix(qkv, out, kcache, vcache, row_off, pre_len, pre_row, pre_pos0, B, Smax, H, smax, kv_tab=None, kv_bs=0):
    """Packed query rows behind a cached prefix: element b = pre_len[b] keys of cache row pre_row[b] from position pre_pos0[b],
    then its rows of qkv (see include/indextts_hip.h)."""
    if not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise NativeError("itts_attn_prefill_prefix: the caches must be contiguous [rows][H][smax][64] views")
    _check(lib().itts_attn_prefill_prefix(_p(qkv), _p(out), _p(kcache), _p(vcache), _p(row_off), _p(pre_len), _p(pre_row),
                                          _p(pre_pos0), B, Smax, H, smax, dt(qkv.dtype), _p(kv_tab), int(kv_bs), _stream()),
           "itts_attn_prefill_prefix")


def attn_prefill_shared(qkv, out, kcache, vcache, row_off, pre_len, pre_row0, w_row, w_pos0, E, Smax, H, smax, kv_tab=None, kv_bs=0):
    """Packed elements behind a prefix block that lives in qkv itself (computed once, shared); own rows appended to the caches
    (see include/indextts_hip.h)."""
    if kcache is not None and not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise NativeError("itts_attn_prefill_shared: the caches must be contiguous [rows][H][smax][64] views")
    _check(lib().itts_attn_prefill_shared(_p(qkv), _p(out), _p(kcache), _p(vcache), _p(row_off), _p(pre_len), _p(pre_row0),
                                          _p(w_row), _p(w_pos0), E, Smax, H, smax, dt(qkv.dtype), _p(kv_tab), int(kv_bs), _stream()),
           "itts_attn_prefill_shared")


def attn_prefill_append(qkv, out, kcache, vcache, row_off, pre_len, w_row, w_pos0, E, Smax, H, smax, kv_tab=None, kv_bs=0):
    """The cached-prefix append form of itts_attn_prefill_shared (pre_row0 = NULL, see include/indextts_hip.h): element e =
    pre_len[e] keys of cache row w_row[e] in front of position w_pos0[e], then its rows of qkv, whose k / v are appended there.
    Checked here, before anything is launched: no paged cache, both caches and w_row / w_pos0 present, contiguous
    [rows][H][smax][64] views of qkv's dtype, Smax >= 1."""
    who = "itts_attn_prefill_shared (append form)"
    if kv_tab is not None:
        raise NativeError(f"{who}: a paged cache (kv_tab) is not supported, pass contiguous caches")
    if kcache is None or vcache is None or w_row is None or w_pos0 is None:
        raise NativeError(f"{who}: the caches, w_row and w_pos0 are required")
    if not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise NativeError(f"{who}: the caches must be contiguous [rows][H][smax][64] views")
    if not (kcache.dtype == vcache.dtype == qkv.dtype == out.dtype):
        raise NativeError(f"{who}: qkv, out and the caches must share one dtype (got {qkv.dtype}, {out.dtype}, {kcache.dtype}, "
                          f"{vcache.dtype})")
    if tuple(kcache.shape[-3:]) != (H, smax, 64) or kcache.shape != vcache.shape:
        raise NativeError(f"{who}: the caches must be [rows][{H}][{smax}][64] (got {tuple(kcache.shape)}, {tuple(vcache.shape)})")
    if int(Smax) < 1:
        raise NativeError(f"{who}: Smax must be at least 1 (got {Smax})")
    _dev(qkv, out, kcache, vcache, row_off, pre_len, w_row, w_pos0)
    _check(lib().itts_attn_prefill_shared(_p(qkv), _p(out), _p(kcache), _p(vcache), _p(row_off), _p(pre_len), None,
                                          _p(w_row), _p(w_pos0), E, Smax, H, smax, dt(qkv.dtype), None, 0, _stream()),
           "itts_attn_prefill_shared")


def kv_share_rows(kc, vc, B, H, Cn, p0, pad, smax, kv_tab=None, kv_bs=0):
    """kc / vc: the whole caches [L, ...] (all layers in one launch): row 0's positions [p0, p0 + Cn) -> [pad[b], pad[b] + Cn) of
    rows 1 .. B-1 (itts_kv_share_rows)."""
    _dev(kc, vc, pad)
    _check(lib().itts_kv_share_rows(_p(kc), _p(vc), kc.shape[0], kc.stride(0), B, H, Cn, p0, _p(pad), smax, _p(kv_tab), int(kv_bs),
                                    dt(kc.dtype), _stream()), "itts_kv_share_rows")


def _sample_args(logits, tokens, history, finished, state, extra_ids, force_stop, stop_token, dbg_scores, no_advance, row_step0):
    """What sample and sample_rows share of itts_sample_args."""
    a = SampleArgs()
    B, V = logits.shape
    a.logits, a.B, a.V, a.ldl = _p(logits), B, V, logits.stride(0)
    a.tokens, a.history, a.hist_cap = _p(tokens), _p(history), history.shape[1]
    a.finished, a.state = _p(finished), _p(state)
    a.extra_ids, a.n_extra = _p(extra_ids), 0 if extra_ids is None else extra_ids.numel()
    a.force_stop, a.stop_token = _p(force_stop), int(stop_token)
    a.dbg_scores, a.no_advance, a.row_step0 = _p(dbg_scores), int(bool(no_advance)), _p(row_step0)
    return a


def sample(logits, tokens, history, finished, state, extra_ids, force_stop, rep_penalty, temperature, top_k, top_p,
           do_sample, seed, stop_token, dbg_scores=None, no_advance=False, row_step0=None):
    a = _sample_args(logits, tokens, history, finished, state, extra_ids, force_stop, stop_token, dbg_scores, no_advance, row_step0)
    a.rep_penalty, a.temperature, a.top_p = float(rep_penalty), float(temperature), float(top_p)
    a.top_k, a.do_sample, a.seed = int(top_k), int(bool(do_sample)), int(seed)
    _check(lib().itts_sample(C.byref(a), _stream()), "itts_sample")


SAMPLE_ROW_BYTES = 32
SAMPLE_MAX_TOP_K = 1024     # the sampler's candidate store
_ROW_KEYS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "seed", "stream")


def check_sample_row(d: dict, what="sampling") -> dict:
    """One row's settings, complete (keys: do_sample, temperature, top_k, top_p, repetition_penalty, seed, stream), checked as
    itts_sample checks its scalars -- ValueError before anything reaches the device.  Returns the normalised dict."""
    unknown = sorted(set(d) - set(_ROW_KEYS))
    missing = sorted(set(_ROW_KEYS) - set(d))
    if unknown or missing:
        raise ValueError(f"{what}: unknown keys {unknown}, missing keys {missing} (a row holds {list(_ROW_KEYS)})")
    r = dict(do_sample=bool(d["do_sample"]), temperature=float(d["temperature"]), top_k=int(d["top_k"]), top_p=float(d["top_p"]),
             repetition_penalty=float(d["repetition_penalty"]), seed=int(d["seed"]) & 0xFFFFFFFFFFFFFFFF,
             stream=int(d["stream"]))
    if not r["repetition_penalty"] > 0.0:
        raise ValueError(f"{what}: repetition_penalty must be positive (got {r['repetition_penalty']})")
    if not 0 <= r["stream"] < (1 << 32):
        raise ValueError(f"{what}: stream must fit 32 bits (got {r['stream']})")
    if r["do_sample"]:
        if not 1 <= r["top_k"] <= SAMPLE_MAX_TOP_K:
            raise ValueError(f"{what}: do_sample needs 1 <= top_k <= {SAMPLE_MAX_TOP_K} (got {r['top_k']}): the device sampler keeps "
                             f"at most {SAMPLE_MAX_TOP_K} candidates per row and refuses to truncate a distribution silently")
        if not 0.0 < r["top_p"] <= 1.0:
            raise ValueError(f"{what}: top_p must lie in (0, 1] (got {r['top_p']})")
        if not r["temperature"] > 0.0:
            raise ValueError(f"{what}: temperature must be positive (got {r['temperature']})")
    else:   # greedy ignores the distribution settings: normalised, as sampling_params does for the scalar form
        r["temperature"], r["top_k"], r["top_p"] = 1.0, 1, 1.0
    return r


def pack_sample_rows(rows):
    """Checked rows (check_sample_row) -> numpy uint8 [len(rows), 32]: the records itts_sample_rows reads (itts_sample_row)."""
    import numpy as np
    recs = (SampleRow * max(len(rows), 1))()
    for rec, d in zip(recs, rows):
        r = check_sample_row(d)
        rec.rep_penalty, rec.temperature, rec.top_p, rec.top_k = r["repetition_penalty"], r["temperature"], r["top_p"], r["top_k"]
        rec.seed, rec.stream, rec.do_sample = r["seed"], r["stream"], int(r["do_sample"])
    return np.frombuffer(bytes(recs), dtype=np.uint8).reshape(-1, SAMPLE_ROW_BYTES)[: len(rows)].copy()


def sample_rows(logits, tokens, history, finished, state, extra_ids, force_stop, rows, stop_token, dbg_scores=None,
                no_advance=False, row_step0=None):
    """itts_sample with per-row settings: rows is a uint8 device tensor [>= B, 32] of packed records (pack_sample_rows: the
    values are checked on the host before the upload, the kernel only guards memory) -- or a list of row dicts, which is
    checked, packed and uploaded here (tests; a captured loop keeps a persistent table)."""
    B, V = logits.shape
    if not torch.is_tensor(rows):
        if len(rows) != B:
            raise ValueError(f"itts_sample_rows: {len(rows)} rows of settings for {B} rows of logits")
        rows = torch.from_numpy(pack_sample_rows(rows)).to(logits.device)
    _dev(rows)
    if rows.dtype != torch.uint8 or rows.numel() < B * SAMPLE_ROW_BYTES:
        raise NativeError("itts_sample_rows: rows must be a uint8 device tensor of B 32-byte records")
    a = _sample_args(logits, tokens, history, finished, state, extra_ids, force_stop, stop_token, dbg_scores, no_advance, row_step0)
    a.rows = _p(rows)
    _check(lib().itts_sample_rows(C.byref(a), _stream()), "itts_sample_rows")


def beam_step(logits, num_beams, tokens, src, beam_scores, hist, hyp_score, hyp_len, hyp_tok, n_hyp, worst, done, state,
              extra_ids, rep_penalty, temperature, top_k, top_p, do_sample, length_penalty, seed, eos_token, scratch=None):
    """logits fp32 [B*num_beams, V]; hist int32 [2, B*num_beams, cap]; see include/indextts_hip.h (itts_beam_args).
    scratch = (cand_scores fp32 [R, BEAM_CAND], cand_ids int32 [R, BEAM_CAND], cand_n int32 [R]) from beam_scratch(R);
    allocated per call when omitted (tests) -- a captured decode loop must pass persistent buffers."""
    a = BeamArgs()
    R, V = logits.shape
    if scratch is None:
        scratch = beam_scratch(R, logits.device)
    cs, cid, cn = scratch
    assert cs.shape[0] >= R and cs.shape[1] == BEAM_CAND and cid.shape == cs.shape and cn.numel() >= R
    a.cand_scores, a.cand_ids, a.cand_n = _p(cs), _p(cid), _p(cn)
    a.logits, a.B, a.num_beams, a.V, a.ldl = _p(logits), R // num_beams, int(num_beams), V, logits.stride(0)
    a.tokens, a.src, a.beam_scores = _p(tokens), _p(src), _p(beam_scores)
    a.hist, a.hist_cap = _p(hist), hist.shape[2]
    a.hyp_score, a.hyp_len, a.hyp_tok, a.n_hyp, a.worst = _p(hyp_score), _p(hyp_len), _p(hyp_tok), _p(n_hyp), _p(worst)
    a.done, a.state = _p(done), _p(state)
    a.extra_ids, a.n_extra = _p(extra_ids), 0 if extra_ids is None else extra_ids.numel()
    a.rep_penalty, a.temperature, a.top_p, a.length_penalty = float(rep_penalty), float(temperature), float(top_p), float(length_penalty)
    a.top_k, a.do_sample, a.seed, a.eos_token = int(top_k), int(bool(do_sample)), int(seed), int(eos_token)
    _check(lib().itts_beam_step(C.byref(a), _stream()), "itts_beam_step")


def beam_scratch(rows, device="cuda"):
    """Scratch between the two launches of a beam step (per-row candidates -> pooling), uninitialised."""
    return (torch.empty(rows, BEAM_CAND, dtype=torch.float32, device=device),
            torch.empty(rows, BEAM_CAND, dtype=torch.int32, device=device),
            torch.empty(rows, dtype=torch.int32, device=device))


def beam_kv_rows(kv_rows, src, state):
    """kv_rows int32 [2][R][smax]: permute the row table by src (call right after beam_step)."""
    _, R, smax = kv_rows.shape
    _check(lib().itts_beam_kv_rows(_p(kv_rows), _p(src), _p(state), R, smax, _stream()), "itts_beam_kv_rows")


def beam_reorder_kv(kc, vc, src, state, B, num_beams):
    """kc / vc: T [L][rows][H][smax][64]; rows of each batch element are permuted in place by src."""
    L, rows, H, smax, hd = kc.shape
    assert hd == 64 and rows >= B * num_beams
    _check(lib().itts_beam_reorder_kv(_p(kc), _p(vc), _p(src), _p(state), L, B, int(num_beams), H, smax, kc.stride(0),
                                      dt(kc.dtype), _stream()), "itts_beam_reorder_kv")


def tanh_pcm(x, wav=None, pcm=None, apply_tanh=True):
    _dev(x)
    _check(lib().itts_tanh_pcm(_p(x), _p(wav), _p(pcm), x.numel(), dt(x.dtype), int(apply_tanh), _stream()),
           "itts_tanh_pcm")
