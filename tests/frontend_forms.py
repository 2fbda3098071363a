"""Form keys of the prompt front-end kernels (csrc/frontend.hip): one pure function per entry point, from the call's arguments to
a small tuple that names the code paths the call takes -- the counterpart of skinny_forms.py.  tests/test_frontend_kernels_gpu.py
adds the key of every case to PINNED and requires the key of every call the two engines make to be in it.  Imports neither torch
nor the native library; every predicate names the line of frontend.hip it mirrors."""


def subsample_conv(T, F, C):
    """("subsample_conv", staged, second channel pass, second frequency pass, waves without channels)."""
    F2 = (F - 3) // 2 + 1
    cpw = (C + 7) // 8                                              # itts_subsample_conv: cpw = (C + 7) / 8 (8 waves of 64)
    staged = C % 8 == 0 and (cpw * F2) % 8 == 0 and C * F2 * 2 <= 64 * 1024      # itts_subsample_conv: `const bool staged = ...`
    return ("subsample_conv", staged,
            cpw > 64,                                               # kernel: `for (cg = c_begin; cg < c_end; cg += 64)` runs twice
            F2 > 64,                                                # kernel: `for (f0 = 0; f0 < F2; f0 += 64)` runs twice
            cpw * 7 >= C)                                           # kernel: `c_begin = wave * cpw` >= C for the last wave


def mha_small(Tq, Tk, H, rel):
    """("mha_small", relpos, steps per wave > 1, ragged last step, ragged query tile)."""
    return ("mha_small", bool(rel),                                 # itts_mha_small: `rel = a->pos != nullptr` picks RELPOS
            Tk > 128,                                               # kernel: `for (kb = wave * 32; kb < Tk; kb += 128)` runs twice in wave 0
            Tk % 32 != 0,                                           # kernel: `key < p.Tk ? ... : -INFINITY` masks inside the last step
            Tq % 16 != 0)                                           # kernel: `if (q0 + r >= p.Tq) return` / the clamped query row


def glu_dwconv_ln_silu(T, C, taps):
    """("glu_dwconv_ln_silu", taps, waves)."""
    return ("glu_dwconv_ln_silu", taps,                             # itts_glu_dwconv_ln_silu: ITTS_DW(7 / 15 / 31)
            C // 128)                                               # block = C / 2 threads: `nw = (blockDim.x + 63) >> 6` entries of red[16]


def rows(M, D, x=False, bias=False, nslab=0, norm=0, y=True, packed=False):
    """("rows", norm, x, bias, slabs, nslab > 8, second column pass, y, packed copy)."""
    return ("rows", int(norm), bool(x), bool(bias), nslab > 0,      # rows_kernel: `p.x != nullptr`, `p.bias != nullptr`, `p.norm`
            nslab > 8,                                              # rows_kernel: `for (s0 = 0; s0 < p.nslab; s0 += 8)` runs twice
            D > 1024,                                               # rows_kernel: `c4 = tid + i * 256 < D4` holds for i = 1
            bool(y), bool(packed))                                  # rows_kernel: `p.y != nullptr`, `p.yp != nullptr`


def col_stats(T, C, mtp, weighted=False, affine=False):
    """("col_stats", weighted, affine, one pass)."""
    return ("col_stats", bool(weighted), bool(affine),              # col_stats_kernel: `wtd = logit != nullptr`, `scale != nullptr`
            mtp <= 32)                                              # col_stats_kernel: `one_pass = mtp <= 8 * NR`


def se_gate(T, C, H, mtp):
    """("se_gate", second k-step per wave, second row-tile pass, second hidden pass, second channel / i0 pass)."""
    return ("se_gate",
            C > 512,                                                # se_gate_kernel: `for (ks = wave; ks < C / 32; ks += 16)` runs twice
            mtp > 4,                                                # se_gate_kernel: `for (mt = 0; mt < mtp; mt += 4)` runs twice
            H > 128,                                                # `for (o = tid >> 3; o < H; o += 128)` and `for (i0 = half * 8; i0 < H; i0 += 128)`
            C > 512)                                                # `for (i0 = part8 * 8; i0 < C; i0 += 512)` and `for (c = tid >> 1; c < C; c += 512)`


def res2_step(T, mtp, chunk, dil, first):
    """("res2_step", first, more than one row tile, ragged last tile)."""
    return ("res2_step", bool(first),                               # res2_step_kernel: `if (p.first)`
            T > 16,                                                 # itts_res2_step: grid (T + 15) / 16
            T % 16 != 0)                                            # res2_step_kernel: `if (row < p.T)` / `min(t0 + r, p.T - 1)`


def im2col_reflect(T, F, taps, dil, Kp):
    """("im2col_reflect", F % 8 != 0, zero columns behind taps * F)."""
    return ("im2col_reflect",
            F % 8 != 0,                                             # im2col_reflect_kernel: an 8-element store straddles two taps (`j = k / F`)
            Kp > taps * F)                                          # im2col_reflect_kernel: `j < taps ? ... : 0.f`


def geglu(M, Kp, mtp):
    return ("geglu",)


def scale_resid(T, C, mtp):
    return ("scale_resid",)
