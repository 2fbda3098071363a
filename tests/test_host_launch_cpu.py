"""The host launchers of csrc/, without a GPU: nothing here reaches a launch.

Plan sweep.  launch_skinny_mt looks the planned (MT, SPW, NTB, FOLD, waves) up among the gemm_skinny_kernel instantiations that are
built and refuses a plan outside that list, so the planner must never name one: every point of the sweep has its form key in
REACHABLE (skinny_forms.py, the list the fp64 pins cover), and the sweep reaches all of REACHABLE.

dtype refusal.  Every exported entry point that takes a dtype goes through one dispatch helper: dtype 7 returns ITTS_ERR_INVALID
with a message that names the entry point, and the 16-bit-only entry points say the same of ITTS_F32.  The list of entry points
is held against _native's prototype table, so a new one has to be classified here before this file passes.
"""
import ctypes as C

import pytest
import torch

from skinny_forms import GEMM_SHAPES, REACHABLE, form_key

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# GEMM_SHAPES: (N, K, ksplit) of the fp64 pins, which reach every form by construction ...
SHAPES = list(GEMM_SHAPES)
# ... and the decode step's own: QKV / out-projection / FC / FC2 / head, with and without the LoRA bank's 128 extra columns
SHAPES += [(n, k, s) for n in (1280, 1344, 3840, 5120, 8194) for k in (1280, 1408, 5120, 5632) for s in (1, 3, 6) if s <= k // 32]
SHAPES = sorted(set(SHAPES))
# (M, rows_per_wg): every M up to 96 with every rows_per_wg; beyond 96 rows with the tiles dealt to grid.z, and chunked
ROWS = [(m, r) for m in range(1, 97) for r in (0, 16, 32)] + [(m, r) for m in (97, 128, 200) for r in (0, 16, 32)]


@pytest.fixture(scope="module")
def nat():
    from indextts import _native
    _native.lib()
    return _native


class RawPlan:
    """nat.skinny_plan's dictionary from one preallocated out8 (the sweep makes ~2 x 10^5 calls)."""

    def __init__(self, nat):
        self.fn, self.dt, self.out = nat.lib().itts_skinny_plan, nat.dt, (C.c_int * 8)()

    def skinny_plan(self, dtype, M, N, K, ksplit=1, rows_per_wg=0, wide_wg=False, fold=False):
        assert self.fn(dtype, M, N, K, ksplit, rows_per_wg, wide_wg, fold, self.out) == 0
        gx, gy, nw, ntb, spw, lds, gz, mt = self.out
        return dict(grid=(gx, gy, gz), waves=nw, tiles_per_wg=ntb, ksteps_per_wave=spw, lds=lds, row_tiles_per_wg=mt)


def test_raw_plan_is_native_skinny_plan(nat):
    raw = RawPlan(nat)
    for args in ((BF16, 13, 4100, 1184, 1, 0, False, True), (F16, 200, 1360, 5248, 3, 16, True, False), (F32, 5, 64, 5248, 1, 0, True, False)):
        assert raw.skinny_plan(nat.dt(args[0]), *args[1:]) == nat.skinny_plan(*args)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_planner_only_names_built_forms(nat, dtype):
    raw, d, seen = RawPlan(nat), nat.dt(dtype), set()
    for N, K, ksplit in SHAPES:
        for fold in ((False, True) if ksplit == 1 else (False,)):
            for wide in (False, True):
                for M, rpw in ROWS:
                    key = form_key(raw, d, M, N, K, ksplit, rpw, wide, fold)
                    assert key in REACHABLE, f"M={M} N={N} K={K} ksplit={ksplit} rows_per_wg={rpw} wide={wide} fold={fold}: {key} is not built"
                    seen.add(key)
    assert REACHABLE - seen == set(), f"forms the sweep never plans: {sorted(REACHABLE - seen)}"


def test_planner_fp32_is_one_row_tile_unfolded(nat):
    fn, out, d = nat.lib().itts_skinny_plan, (C.c_int * 8)(), nat.dt(F32)
    for N, K, ksplit in SHAPES:
        for fold in ((0, 1) if ksplit == 1 else (0,)):
            for wide in (0, 1):
                for M, rpw in ROWS:
                    assert fn(d, M, N, K, ksplit, rpw, wide, fold, out) == 0
                    gx, gy, nw, ntb, spw, lds, gz, mt = out
                    # one row tile; no LayerNorm statistics in LDS: the accumulator exchange alone (1 KiB per wave and column tile)
                    assert mt == 1 and gz == 1 and lds == max(1024, nw * ntb * 1024) and \
                        (1, 5 if spw <= 5 else 10, ntb, False, 16 if nw == 16 else 8) in REACHABLE, \
                        f"M={M} N={N} K={K} ksplit={ksplit} rows_per_wg={rpw} wide={wide} fold={fold}: {list(out)}"


def test_planner_fp32_wide_names_the_16_wave_form(nat):
    """fp32 with wide_wg and more than 80 k-steps per slice: the launcher runs <1, 10, 1, false, 16> (16 waves, one column tile,
    16 KiB of LDS), and the plan says so; at 80 k-steps or fewer, and in every folded or many-row-tile launch, 8 waves."""
    assert form_key(nat, F32, 5, 64, 5248, wide=True) == (1, 10, 1, False, 16)
    p = nat.skinny_plan(F32, 5, 64, 5248, 1, 0, True, False)
    assert p["waves"] == 16 and p["tiles_per_wg"] == 1 and p["lds"] == 16384 and p["ksteps_per_wave"] == 21
    assert form_key(nat, F32, 5, 64, 5248, wide=False)[4] == 8 and form_key(nat, F32, 5, 64, 1280, wide=True)[4] == 8
    assert form_key(nat, BF16, 5, 64, 5248, wide=True) == (1, 10, 1, False, 16) and form_key(nat, BF16, 5, 64, 2560, wide=True)[4] == 8


# ---------------------------------------------------------------------------------------------------------- dtype refusal
P = 0x1000                                   # never dereferenced: every call below is refused before a launch
FIR = (C.c_float * 12)()                     # itts_aa_snake_fwd copies its two filters on the host before it looks at dtype
FIRP = C.cast(FIR, C.c_void_p)


def struct(cls, **kw):
    a = cls()
    for k, v in kw.items():
        setattr(a, k, v)
    return C.byref(a)


def calls(nat):
    """name -> (dtype -> return code), with arguments that pass every check in front of the dtype dispatch; "name/what" is a
    second dispatch site of the same entry point."""
    L = nat.lib()
    SEG = struct(nat.SegTableArgs, dev=P, host=P, nseg=1, ntiles=1)   # (the table is looked at behind the dtype dispatch)
    return {
        "itts_pack_weight": lambda d: L.itts_pack_weight(P, P, 1, 64, 64, d, None),
        "itts_aa_snake_fwd": lambda d: L.itts_aa_snake_fwd(P, P, P, P, FIRP, FIRP, 1, 64, 32, d, 0, None, None),
        "itts_aa_snake_fwd/layout 1": lambda d: L.itts_aa_snake_fwd(P, P, P, P, FIRP, FIRP, 1, 64, 32, d, 1, None, None),
        "itts_gemm_skinny": lambda d: L.itts_gemm_skinny(struct(nat.SkinnyArgs, dtype=d, M=4, N=64, K=64, wp=P, x=P, y=P, epi=nat.EPI_STORE), None),
        "itts_skinny_plan": lambda d: L.itts_skinny_plan(d, 4, 64, 64, 1, 0, 0, 0, (C.c_int * 8)()),
        "itts_gemm_conv": lambda d: L.itts_gemm_conv(struct(nat.ConvArgs, dtype=d, B=1, Tin=16, Tout=16, Cin=64, N=64, taps=1, dil=1, x=P, wp=P, y=P), None),
        "itts_layernorm": lambda d: L.itts_layernorm(P, P, P, None, None, P, 0, 4, 64, d, None),
        "itts_ln_reduce": lambda d: L.itts_ln_reduce(struct(nat.LnReduceArgs, dtype=d, M=4, D=256, h=P, w=P, b=P, y=P), None),
        "itts_lora_shrink": lambda d: L.itts_lora_shrink(struct(nat.LoraShrinkArgs, dtype=d, M=4, K=64, x=P, ids=P, a_bank=P, u=P, n=3, rp=16, Kx=64, ldu=128), None),
        "itts_embed_step": lambda d: L.itts_embed_step(P, P, P, P, 0, P, 4, 64, None, None, 8, None, d, None),
        "itts_attn_decode": lambda d: L.itts_attn_decode(P, P, P, P, P, P, 2, 2, 64, d, 0, None, None, None, None, None, 0, None),
        "itts_attn_prefill": lambda d: L.itts_attn_prefill(P, P, P, P, P, 1, 8, 2, 64, d, None),
        "itts_attn_prefill_packed": lambda d: L.itts_attn_prefill_packed(P, P, P, P, P, None, 1, 8, 2, 64, d, None, 0, None),
        "itts_attn_prefill_prefix": lambda d: L.itts_attn_prefill_prefix(P, P, P, P, P, P, P, P, 1, 8, 2, 64, d, None, 0, None),
        "itts_attn_prefill_shared": lambda d: L.itts_attn_prefill_shared(P, P, P, P, P, P, P, P, P, 1, 8, 2, 64, d, None, 0, None),
        "itts_kv_share_rows": lambda d: L.itts_kv_share_rows(P, P, 1, 1024, 2, 2, 4, 0, P, 64, None, 0, d, None),
        "itts_beam_reorder_kv": lambda d: L.itts_beam_reorder_kv(P, P, P, P, 1, 1, 2, 2, 64, 1024, d, None),
        "itts_tanh_pcm": lambda d: L.itts_tanh_pcm(P, P, None, 16, d, 0, None),
        "itts_lora_shrink_mix": lambda d: L.itts_lora_shrink_mix(struct(nat.LoraShrinkArgs, dtype=d, M=4, K=64, x=P, mix=P, a_bank=P, u=P, n=3, rp=16, Kx=64, ldu=128), None),
        "itts_refill_join": lambda d: L.itts_refill_join(struct(nat.RefillJoinArgs, dtype=d, L=1, H=1, hist_cap=8), None),
        # ---- FP8 weights: the activation type is bf16 / f16
        "itts_gemm_skinny_w8": lambda d: L.itts_gemm_skinny_w8(struct(nat.SkinnyArgs, dtype=d, M=4, N=64, K=64, wp=P, x=P, y=P, w_scale=P, epi=nat.EPI_STORE), None),
        "itts_skinny_plan_w8": lambda d: L.itts_skinny_plan_w8(d, 4, 64, 64, 0, 0, (C.c_int * 8)()),
        # ---- built for bf16 / f16 only
        "itts_subsample_conv": lambda d: L.itts_subsample_conv(P, P, P, P, 8, 8, 8, d, None),
        "itts_mha_small": lambda d: L.itts_mha_small(struct(nat.MhaArgs, dtype=d, Tq=4, Tk=4, H=1, q=P, k=P, v=P, out=P, q_stride=64, k_stride=64, v_stride=64, out_mtp=1), None),
        "itts_glu_dwconv_ln_silu": lambda d: L.itts_glu_dwconv_ln_silu(P, P, P, P, P, P, 4, 128, 15, 1, 1e-5, d, None),
        "itts_rows": lambda d: L.itts_rows(struct(nat.RowsArgs, dtype=d, M=4, D=64, x=P, y=P, y_packed=P), None),
        "itts_geglu": lambda d: L.itts_geglu(P, P, 4, 64, 0, d, None),
        "itts_im2col_reflect": lambda d: L.itts_im2col_reflect(P, P, 8, 8, 3, 1, 32, 1, d, None),
        "itts_res2_step": lambda d: L.itts_res2_step(P, P, P, P, P, P, 8, 1, 1, 1, 1, d, None),
        "itts_se_gate": lambda d: L.itts_se_gate(P, P, P, P, P, P, 8, 64, 16, 1, d, None),
        "itts_scale_resid": lambda d: L.itts_scale_resid(P, P, P, P, 8, 32, 1, d, None),
        "itts_col_stats": lambda d: L.itts_col_stats(P, None, None, None, P, 8, 64, 1, d, None),
        "itts_attn_decode_kv8": lambda d: L.itts_attn_decode_kv8(P, P, P, P, P, P, P, 2, 2, d, 0, None, P, 16, None),
        "itts_kv8_store": lambda d: L.itts_kv8_store(P, P, P, P, None, None, None, 2, 8, 2, d, P, 16, None),
        "itts_subsample_conv_seg": lambda d: L.itts_subsample_conv_seg(P, P, P, P, SEG, 8, 8, 8, d, None),
        "itts_mha_small_seg": lambda d: L.itts_mha_small_seg(struct(nat.MhaArgs, dtype=d, Tq=4, Tk=4, H=1, q=P, k=P, v=P, out=P, q_stride=64, k_stride=64, v_stride=64, out_mtp=1), SEG, 0, None),
        "itts_glu_dwconv_ln_silu_seg": lambda d: L.itts_glu_dwconv_ln_silu_seg(P, P, P, P, P, P, SEG, 128, 15, 1, 1e-5, d, None),
    }


ONLY_16BIT = ("itts_subsample_conv", "itts_mha_small", "itts_glu_dwconv_ln_silu", "itts_rows", "itts_geglu", "itts_im2col_reflect",
              "itts_res2_step", "itts_se_gate", "itts_scale_resid", "itts_col_stats", "itts_attn_decode_kv8", "itts_kv8_store",
              "itts_subsample_conv_seg", "itts_mha_small_seg", "itts_glu_dwconv_ln_silu_seg")
# FP8 weights under 16-bit activations: these two word their refusal of ITTS_F32 (and of any other dtype) themselves
ACT_16BIT = ("itts_gemm_skinny_w8", "itts_skinny_plan_w8")
ACT_16BIT_SAYS = "the activation type must be bf16 or f16"
# no dtype among the arguments -- or, itts_packed_bytes, one that only sizes a buffer: it returns a byte count, not a status
NO_DTYPE = ("itts_abi_version", "itts_last_error", "itts_last_kernel", "itts_packed_bytes", "itts_sample", "itts_beam_step",
            "itts_beam_kv_rows", "itts_prefix_rows", "itts_packed_bytes_w8", "itts_pack_weight_w8", "itts_sample_rows")
# the three prefill variants run the launcher of itts_attn_prefill, which reports under that name
REPORTS_AS = {"itts_attn_prefill_packed": "itts_attn_prefill", "itts_attn_prefill_prefix": "itts_attn_prefill",
              "itts_attn_prefill_shared": "itts_attn_prefill"}


def test_every_entry_point_is_classified(nat):
    table = {name.split("/")[0] for name in calls(nat)}
    assert set(table) | set(NO_DTYPE) == set(nat.EXPORTED_SYMBOLS) and not set(table) & set(NO_DTYPE)
    assert set(ONLY_16BIT) <= set(table) and set(ACT_16BIT) <= set(table) and not set(ONLY_16BIT) & set(ACT_16BIT)


def test_unknown_dtype_is_refused_by_name(nat):
    L = nat.lib()
    for name, call in calls(nat).items():
        assert call(7) == 1, (name, L.itts_last_error())
        err = L.itts_last_error().decode()
        entry = name.split("/")[0]
        assert err.startswith(REPORTS_AS.get(entry, entry) + ":"), (name, err)


def test_fp32_is_refused_by_the_16_bit_entry_points(nat):
    L, table = nat.lib(), calls(nat)
    for name in ONLY_16BIT:
        assert table[name](nat.dt(F32)) == 1, (name, L.itts_last_error())
        err = L.itts_last_error().decode()
        assert err.startswith(name + ":") and "bf16 / f16" in err, (name, err)


def test_fp32_is_refused_by_the_fp8_weight_entry_points(nat):
    L, table = nat.lib(), calls(nat)
    for name in ACT_16BIT:
        for d in (nat.dt(F32), 7):
            assert table[name](d) == 1, (name, L.itts_last_error())
            err = L.itts_last_error().decode()
            assert err.startswith(name + ":") and ACT_16BIT_SAYS in err, (name, err)
