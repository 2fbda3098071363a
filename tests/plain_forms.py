"""Kernel forms of itts_gemm_conv at taps = 1 (csrc/gemm_conv.hip, dispatch_conv): one pure function from a call's shape to the form
string itts_last_kernel() reports, and the launch arithmetic the fp64 pins (tests/test_plain_gemm_kernels_gpu.py) choose their
shapes by -- the counterpart of skinny_forms.py and frontend_forms.py.  Imports neither torch nor the native library; every
predicate names the line of gemm_conv.hip it mirrors.  The narrow forms (Cin <= 64 and N <= 64) are the vocoder file's: `form`
refuses such a shape."""

TAGS = ("bf16", "f16", "f32")


def kstep(tag):
    """K extent of one k-step: Elem<T>::KS."""
    return 16 if tag == "f32" else 32


def rounds(mb, nb, cus):
    """dispatch_conv: rounds of the chip over its 2 * CUs workgroup slots."""
    slots = 2 * cus
    return (mb * nb + slots - 1) // slots


def wide_tiles(M, N, cus):
    """dispatch_conv: `if (5 * r160 < 4 * r128)` -- 128 x 160 tiles where they save a round."""
    mb = (M + 127) // 128
    return N % 160 == 0 and 5 * rounds(mb, N // 160, cus) < 4 * rounds(mb, N // 128, cus)


def first_wide_mblocks(N, cus):
    """The smallest number of 128-row blocks at which an N-column plain GEMM takes the 128 x 160 form."""
    mb = 1
    while not wide_tiles(mb * 128, N, cus):
        mb += 1
    return mb


def form(tag, B, M, N, K, ksplit=1, cus=256):
    """The form string of itts_gemm_conv(taps = 1) at this shape on a part with `cus` compute units."""
    assert tag in TAGS and not (K <= 64 and N <= 64), "dispatch_narrow takes Cin <= 64 with N <= 64"
    if N % 128 == 0:                                                 # `if (plain && p.N % 128 == 0)`
        if ksplit <= 1 and B == 1 and wide_tiles(M, N, cus):          # `if (p.ksplit <= 1 && p.N % 160 == 0 && p.B == 1)`
            return f"gemm_plain<{tag},4,2,2,5>"
        return f"gemm_plain<{tag},2,4,4,2>"
    if N % 64 == 0:                                                  # `if (plain && p.N % 64 == 0)`
        rows = B * ((M + 255) // 256)
        return f"gemm_conv<{tag},4,2,4,2,4,0>" if rows * (N // 64) >= 448 else f"gemm_conv<{tag},4,2,2,2,4,0>"
    if N % 96 == 0:                                                  # the convolution forms with taps = 1 (HALO = CV_MAX_HALO = 64)
        return f"gemm_conv<{tag},2,2,4,3,2,64,persist>"
    if N % 48 == 0:
        return f"gemm_conv<{tag},4,1,4,3,2,64>"
    return f"gemm_conv<{tag},4,1,4,2,2,64>"


def l2_patch_gm(BN, KT):
    """l2_patch_gm(BN, KT, taps = 1): m-blocks per L2 patch of tile_of_workgroup."""
    wbytes = BN * KT * 64
    gn = min(8, max(1, (2 << 20) // max(wbytes, 1)))
    gm = 32 // gn
    return 32 if gm >= 32 else 16 if gm >= 16 else 8 if gm >= 8 else 4


def slice_ksteps(KT, ks, s):
    """gemm_plain_kernel: k-steps [kt0, kt1) of split-K slice s -- `kt0 = (b * KT) / ksplit`."""
    return (s * KT) // ks, ((s + 1) * KT) // ks


# Every form string dispatch_conv can return for taps = 1 (the narrow forms aside), for the three dtypes
REACHABLE = {f"{base}<{tag},{params}>" for tag in TAGS for base, params in (
    ("gemm_plain", "2,4,4,2"), ("gemm_plain", "4,2,2,5"), ("gemm_conv", "4,2,4,2,4,0"), ("gemm_conv", "4,2,2,2,4,0"),
    ("gemm_conv", "2,2,4,3,2,64,persist"), ("gemm_conv", "4,1,4,3,2,64"), ("gemm_conv", "4,1,4,2,2,64"))}
