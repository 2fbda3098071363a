"""The gemm_skinny_kernel instantiations a plan can name: shared by the fp64 pins (test_decode_kernels_gpu.py) and the planner
sweep (test_host_launch_cpu.py).  Imports neither torch nor the native library."""


def form_key(nat, dtype, M, N, K, ksplit=1, rows_per_wg=0, wide=False, fold=False):
    """(MT, SPW, NTB, FOLD, MAXW) of the gemm_skinny_kernel instantiation a launch of this shape runs."""
    p = nat.skinny_plan(dtype, M, N, K, ksplit, rows_per_wg, wide, fold)
    return (p["row_tiles_per_wg"], 5 if p["ksteps_per_wave"] <= 5 else 10, p["tiles_per_wg"], bool(fold), 16 if p["waves"] == 16 else 8)


# Every instantiation launch_skinny_mt can be asked for, by plan_skinny's rules:
#   SPW 5:  NTB 1, 2, 3 -- 3 not with FOLD and MT > 2 (the statistics accumulators: demoted to 2) --, and NTB 4 only with FOLD and MT <= 2;
#   SPW 10: NTB 1, and NTB 2 only with MT <= 2 (4-6 row tiles with 10-step chunks: accumulators + weight fragments);
#   16 waves: MT 1, not folded, always <10, 1, 16>.
# Anything else is not built: launch_skinny_mt looks the plan up in this list, and a plan outside it (NTB 3 with FOLD and MT > 2,
# NTB 4 without FOLD or with MT > 2, SPW 10 with NTB 2 and MT > 2, a 16-wave folded form, MT 3 / 5) is an error that names the
# plan and launches nothing.  33-64 rows run MT 4 with tiles that may be empty, 65-96 rows MT 6.
REACHABLE = set()
for _mt in (1, 2, 4, 6):
    for _fold in (False, True):
        for _ntb in (1, 2, 3, 4):
            if (_ntb == 3 and _fold and _mt > 2) or (_ntb == 4 and not (_fold and _mt <= 2)):
                continue
            REACHABLE.add((_mt, 5, _ntb, _fold, 8))
        REACHABLE.add((_mt, 10, 1, _fold, 8))
        if _mt <= 2:
            REACHABLE.add((_mt, 10, 2, _fold, 8))
REACHABLE.add((1, 10, 1, False, 16))


# (N, K, ksplit) of GEMM_CASES in test_decode_kernels_gpu.py (which holds its cases against this list): the shapes at which the
# fp64 pins reach every form, and the planner sweep's starting point
GEMM_SHAPES = [
    (50, 96, 1), (50, 1184, 1), (50, 1408, 1), (50, 2720, 1), (50, 5248, 1), (64, 96, 1), (64, 320, 1), (64, 1184, 1), (64, 1280, 1),
    (64, 1408, 1), (64, 2720, 1), (64, 5248, 1), (272, 1312, 1), (272, 1408, 1), (272, 1408, 2), (384, 96, 1), (384, 1184, 1),
    (384, 1280, 1), (384, 1408, 1), (528, 96, 1), (528, 1280, 1), (528, 1312, 1), (528, 2720, 1), (608, 1184, 1), (784, 1280, 1),
    (800, 1184, 1), (1040, 96, 1), (1040, 160, 4), (1040, 1184, 4), (1360, 320, 1), (1360, 5248, 3), (2064, 160, 4), (2080, 1184, 1),
    (4100, 1184, 1), (4100, 1280, 1), (4112, 1184, 1), (4112, 1408, 1), (4128, 1280, 1), (8194, 160, 1), (8194, 1408, 1),
    (8194, 5248, 1), (8196, 320, 1)]


# fp32 (Elem<float>: KS = 16): launch_skinny refuses the folded form and builds MT = 1 only -- the entry point cuts the rows 16 at a
# time (skinny_row_tiles) --, so plan_skinny's rules leave  SPW 5 with NTB 1, 2, 3;  SPW 10 with NTB 1, 2;  16 waves: <10, 1, 16>.
REACHABLE_F32 = {(1, 5, _ntb, False, 8) for _ntb in (1, 2, 3)} | {(1, 10, _ntb, False, 8) for _ntb in (1, 2)} | {(1, 10, 1, False, 16)}
assert REACHABLE_F32 <= REACHABLE

# K of the fp32 pins (tests/test_fp32_kernels_gpu.py), in k-steps of 16: 1; 6; 40 | 41 (SPW 5 -> 10); 80 (one 10-step pass of every
# wave); 81 (a second pass of one step); 320 (four passes).  The N with 2 and 3 column tiles per workgroup come from skinny_plan.
F32_K = (16, 96, 640, 656, 1280, 1296, 5120)
F32_N = (50, 64)
F32_M = (1, 13, 16, 17, 32, 33)


def first_n_with_tiles(nat, dtype, ntb, K=16):
    """The smallest N for which skinny_plan gives a workgroup `ntb` column tiles (K = 16: one k-step, the SPW 5 form)."""
    for nt in range(1, 4097):
        N = (nt - 1) * 16 + 1
        if nat.skinny_plan(dtype, 1, N, K)["tiles_per_wg"] >= ntb:
            return N
    raise AssertionError(f"no N up to 65521 plans {ntb} column tiles per workgroup")
