/*
 * indextts_hip_w8.h -- FP8 (OCP E4M3, "e4m3fn") weight-only forms of the decode-step GEMM.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  The Python side lists these entry points as _native.W8_SYMBOLS (tests/test_w8_cpu.py holds the list against
 * the library's exports).
 *
 * Scheme.  A weight matrix W[K][N] is stored as one E4M3 code per element plus one fp32 scale per output column:
 *     W[k][n] ~ w_scale[n] * decode(code[k][n]),   w_scale[n] = max_k |W[k][n]| / 448   (indextts/utils/quant.py).
 * Codes are OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7f / 0xff are NaN and never produced by
 * the quantiser (the kernel does not treat them specially: they must not be fed).  Activations,
 * accumulation (fp32), the KV cache, the LayerNorm statistics and every epilogue stay as in the 16-bit kernel: a code is
 * converted IN REGISTERS to the activation type T (bf16 or f16; exact, every finite E4M3 value -- subnormals included -- is
 * representable in both) and feeds the same 16x16x32 MFMA as the A operand.
 *
 * Packed FP8 weight layout.  1-KiB blocks, each 16 columns x 64 k:
 *     block(nt, kb),  nt = n / 16 in [0, ceil(N / 16)),  kb = k / 64 in [0, ceil(K / 64)),  at byte ((nt * KB + kb) * 1024),
 *                     KB = ceil(K / 64); zero codes (0x00) pad K to a multiple of 64 and N to a multiple of 16.
 *     inside a block: lane l = (g << 4) | c (g = 0..3, c = 0..15) owns 16 contiguous bytes:
 *                     byte e     (e = 0..7) = code[kb * 64      + g * 8 + e][nt * 16 + c]
 *                     byte 8 + e (e = 0..7) = code[kb * 64 + 32 + g * 8 + e][nt * 16 + c]
 * i.e. the low 8 bytes are lane l's fragment of the 32-k step 2 kb and the high 8 bytes its fragment of step 2 kb + 1, in the k
 * order of the 16-bit packed weight layout and of the packed activation layout (lane (g, r) of k-step s holds k = 32 s + 8 g +
 * 0..7): one 16-byte load per lane yields the two complete 16x16x32 A fragments the 16-bit kernel loads as two blocks, and the
 * activations are read unchanged.
 */
#ifndef INDEXTTS_HIP_W8_H
#define INDEXTTS_HIP_W8_H

/* bytes of the packed image: ceil(N / 16) * ceil(K / 64) * 1024 */
int64_t itts_packed_bytes_w8(int K, int N);
/* codes uint8 [K][N] row-major (device) -> packed (device), the layout above */
int itts_pack_weight_w8(const void* codes, void* packed, int K, int N, void* stream);

/* Y[M][N] = epi( w_scale[n] * (X[M][K] @ decode(codes)[K][N]) + bias ): itts_gemm_skinny over FP8 weights.  Fields as in
 * itts_skinny_args (indextts_hip.h) where they apply.  Epilogue order: the accumulator is multiplied by w_scale[n] FIRST, then
 * everything the 16-bit epilogue does; LayerNorm folded (ln_c != NULL):
 *     v = rstd[m] * ( w_scale[n] * acc[m][n] - mean[m] * ln_c[n] ) + bias[n],   ln_c[n] = w_scale[n] * sum_k decode(code[k][n])
 * (the caller sums in float64), so a constant row cancels as in the 16-bit form.
 * dtype: ITTS_BF16 or ITTS_F16 (the activation type; ITTS_F32 is refused).  Epilogues: ITTS_EPI_STORE, _GELU_STORE, _RESID_F32,
 * _QKV_CACHE, _STORE_F32 (what the "fold" decode step and the head use); the split-K slab, _SILU_STORE and the
 * ITTS_EPI_RELU_AFFINE_* epilogues are refused, as is ksplit > 1.
 * K % 32 == 0 (the activations' k-steps; the weight image is padded to 64).  Up to 96 rows per launch; more rows go 96 at a time
 * or, with rows_per_wg > 0, in one launch whose row tiles are dealt to grid.z. */
typedef struct itts_skinny_w8_args {
  int dtype;
  int M, N, K;
  const void* wp;       /* packed E4M3 codes (itts_pack_weight_w8) */
  const float* w_scale; /* [N] */
  const float* bias;    /* [N] or NULL */
  const void* x;        /* T [M][K] */
  int epi;
  void* y;
  float* yf;
  void* kcache;
  void* vcache;
  const int32_t* pos;
  int heads, smax;
  int ksplit; /* 0 / 1 only */
  const float* ln_c;
  float ln_eps;
  int32_t* bump;
  int rows_per_wg;
  const int32_t* kv_tab;
  int kv_bs;
  int x_packed, y_packed;
  int y_row0, y_mtp, x_mtp;
} itts_skinny_w8_args;
int itts_gemm_skinny_w8(const itts_skinny_w8_args* a, void* stream);
/* launch geometry itts_gemm_skinny_w8 would use: out8 = {grid.x, grid.y, waves per workgroup, column tiles per workgroup,
 * 64-k weight blocks per wave, dynamic LDS bytes, grid.z, row tiles per workgroup} (host-only, launches nothing) */
int itts_skinny_plan_w8(int dtype, int M, int N, int K, int rows_per_wg, int fold, int* out8);

#endif
