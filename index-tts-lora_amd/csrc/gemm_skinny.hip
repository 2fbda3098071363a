// Skinny (decode-step) GEMM: Y[M<=96][N] = epi( X[M][K] @ W[K][N] + bias ).
//
// HBM-bound weight streaming, latency-first structure: every global load a wave needs (its 1-KiB packed weight blocks,
// straight into MFMA operand registers, and its fragments of the T-typed activations) is issued BEFORE the first use, so
// a launch costs one memory round trip plus the stream time.  A workgroup owns 1-3 16-column tiles and one slice of K
// (grid.y = split-K factor); its waves split that slice and their fp32 partial tiles are summed through LDS in a FIXED
// order.  The MFMAs run with the WEIGHT fragment as the A operand: the accumulator tile comes out transposed, a lane
// holds FOUR CONSECUTIVE OUTPUT COLUMNS of one batch row, and every epilogue access is 8 or 16 bytes wide.
// Up to 96 rows (6 row tiles) share one pass over the weights: batch 32 x 3 beams (the infer() default) or several pooled
// requests read the 966 MB of decoder weights ONCE per token.
//
// With split-K > 1 each slice stores its partial tile into its own fp32 slab [ks][M][N]; the next launch (itts_ln_reduce)
// sums the slabs in a fixed order.
//
// LayerNorm folded into the consumer (FOLD, round 4): the QKV and FC projections of a block consume LN(h).  With
//   LN(h) W + b = rstd (h (gamma . W) - mean c) + d,   c_j = sum_k gamma_k W_kj,   d_j = sum_k beta_k W_kj + b_j
// (gamma . W packed at load time, c and d fp32 vectors) the GEMM multiplies the RAW residual rows -- a T-typed packed copy
// of h that the producing launch's residual epilogue writes -- and needs the row statistics only in its EPILOGUE.  They
// come from the matrix pipe, off the fragments the wave holds anyway: sum h = ones x frag, sum h^2 = diagonal of frag x
// frag (the 16 x 16 Gram tile of the row tile), accumulated in fp32 over the wave's K share and reduced across the waves
// together with the partial tiles.  Every workgroup covers the whole K, so every workgroup has the full statistics of
// all its rows: no cross-workgroup hand-off, no [residual-reduce + LayerNorm] launch in front of the GEMM.  The
// producers (attention out-projection, FC2) run without split-K and add into the fp32 residual stream in their epilogue
// (one owner per element: deterministic) and also store the T-typed packed copy.  A block is 5 launches instead of 7.
// Replaces the per-step Conv1D/Linear (+ residual + LayerNorm) calls of HF GPT2Block as driven by
// indextts/gpt/model.py:163-193.
#include "gemm_skinny_kernel.h"

namespace itts {

#if ITTS_STAMPS
unsigned long long* g_stamp_buf = nullptr;
unsigned long long* g_stamp_buf_sample = nullptr;
#endif

#if ITTS_DIAG
int g_tune_ntb = 0, g_tune_nw = 0;  // diagnostic build: itts_debug_set(1|2, v) overrides (0 = heuristic)
int g_skinny_exp = 0;               // itts_debug_set(6, bits): load ablations of the skinny GEMM (SkinnyParams::exp)
#endif

static int skinny_no_form(const SkinnyPlan& q, bool fold) {
  set_error("itts_gemm_skinny: no form <%d,%d,%d,%d,%d> is built", q.MT, q.SPWc, q.ntb, (int)fold, q.NW);
  return ITTS_ERR_INVALID;
}

// Looks the planned (SPWc, ntb, 8 | 16 waves) up among the instantiations that exist for this (T, MT, FOLD): the same list as
// plan_skinny's register-budget rules.  A plan outside it launches nothing.
template <typename T, int MT, bool FOLD>
static int launch_skinny_mt(const SkinnyParams& p, const SkinnyPlan& q, hipStream_t s) {
  dim3 grid(q.gx, q.gy, q.gz), block(q.NW * 64);
  const int maxw = q.NW == 16 ? 16 : 8;
#define ITTS_SK(SPW_, NTB_, MAXW_)                                                                         \
  if (q.SPWc == SPW_ && q.ntb == NTB_ && maxw == MAXW_) {                                                  \
    hipLaunchKernelGGL((gemm_skinny_kernel<T, MT, SPW_, NTB_, FOLD, MAXW_>), grid, block, q.lds, s, SKINNY_LEAD_ARGS(p, q), static_cast<const SkinnyTail&>(p));    \
    return check_launch("itts_gemm_skinny");                                                               \
  }
  ITTS_SK(5, 1, 8)
  ITTS_SK(5, 2, 8)
  if constexpr (!(FOLD && MT > 2)) ITTS_SK(5, 3, 8)    // the statistics accumulators take 8 registers per row tile
  if constexpr (FOLD && MT <= 2) ITTS_SK(5, 4, 8)
  ITTS_SK(10, 1, 8)
  if constexpr (MT <= 2) ITTS_SK(10, 2, 8)
  if constexpr (MT == 1 && !FOLD) ITTS_SK(10, 1, 16)
#undef ITTS_SK
  return skinny_no_form(q, FOLD);
}

template <typename T>
static int launch_skinny(const SkinnyParams& p, const SkinnyPlan& q, hipStream_t s) {
  const bool fold = p.cvec != nullptr;
  if constexpr (sizeof(T) == 4) {
    if (fold) {
      set_error("itts_gemm_skinny: the LayerNorm-folded form is built for bf16 / f16");
      return ITTS_ERR_INVALID;
    }
    if (q.MT == 1) return launch_skinny_mt<T, 1, false>(p, q, s);
  } else {
    switch (q.MT) {
#define ITTS_MT(MT_) \
  case MT_: return fold ? launch_skinny_mt<T, MT_, true>(p, q, s) : launch_skinny_mt<T, MT_, false>(p, q, s)
      ITTS_MT(1);
      ITTS_MT(2);
      ITTS_MT(4);
      ITTS_MT(6);
#undef ITTS_MT
    }
  }
  return skinny_no_form(q, fold);
}

}  // namespace itts

using namespace itts;

extern "C" int itts_gemm_skinny(const itts_skinny_args* a, void* stream) {
  int ksplit, y_mtp, kv_bs_log2;
  if (int rc = skinny_check(a, "itts_gemm_skinny", false, &ksplit, &y_mtp, &kv_bs_log2)) return rc;
  const size_t esz = a->dtype == ITTS_F32 ? 4 : 2;
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0, rows = 0; r0 < a->M; r0 += rows) {
    const int MTall = skinny_row_tiles(a->dtype, a->M - r0, a->rows_per_wg, &rows);
    SkinnyParams p = skinny_params_of(a, r0, rows, esz, y_mtp, kv_bs_log2);
    p.ksplit = ksplit;
#if ITTS_STAMPS
    p.stamps = g_stamp_buf;
#endif
#if ITTS_DIAG
    p.exp = g_skinny_exp;
#endif
    const int rc = by_dtype(a->dtype, "itts_gemm_skinny", [&](auto tag) {
      using T = typename decltype(tag)::type;
      return launch_skinny<T>(p, plan_skinny(skinny_walk<T>(p.K), p.N, p.ksplit, MTall, a->rows_per_wg, a->wide_wg != 0, p.cvec != nullptr), s);
    });
    if (rc != ITTS_OK) return rc;
  }
  return ITTS_OK;
}

extern "C" int itts_skinny_plan(int dtype, int M, int N, int K, int ksplit, int rows_per_wg, int wide_wg, int fold, int* out8) {
  ITTS_REQUIRE(out8 && N > 0 && K > 0 && ksplit > 0 && M > 0, "itts_skinny_plan: bad arguments");
  int rows;
  const int MTall = skinny_row_tiles(dtype, M, rows_per_wg, &rows);   // (of the first launch, when the rows take several)
  return by_dtype(dtype, "itts_skinny_plan", [&](auto tag) {
    using T = typename decltype(tag)::type;
    return skinny_plan_out8(plan_skinny(skinny_walk<T>(K), N, ksplit, MTall, rows_per_wg, wide_wg != 0, fold != 0), out8);
  });
}

#if ITTS_DIAG
// ---- diagnostic build only (libindextts_hip_diag.so, include/indextts_hip_diag.h); absent from the product library
namespace itts { extern int g_conv_cfg; extern int g_attn_waves; extern int g_attn_full_pass;
                 extern unsigned long long* g_stamp_buf_attn; int g_stamp_target = 0; }

extern "C" int itts_debug_set(int key, int value) {
  if (key == 1) itts::g_tune_ntb = value;
  else if (key == 2) itts::g_tune_nw = value;
  else if (key == 3) itts::g_conv_cfg = value;
  else if (key == 4) itts::g_attn_waves = (value == 8) ? 8 : 4;
  else if (key == 6) itts::g_skinny_exp = value;
  else if (key == 7) itts::g_attn_full_pass = value != 0;
  else if (key == 8) itts::g_stamp_target = value == 1;
  else return ITTS_ERR_INVALID;
  return ITTS_OK;
}

// every later itts_gemm_skinny launch writes 16 u64 per workgroup to `buf` (NULL switches it off)
extern "C" int itts_debug_stamps(void* buf) {
#if ITTS_STAMPS
  if (itts::g_stamp_target == 1) itts::g_stamp_buf_attn = (unsigned long long*)buf;   // itts_debug_set(8, 1): attn_decode_kernel
  else itts::g_stamp_buf = (unsigned long long*)buf;
  return ITTS_OK;
#else
  (void)buf;
  return ITTS_ERR_INVALID;
#endif
}

// the same for the tiled convolution kernel: 16 x u64 per workgroup (tools/timeline_conv.py)
namespace itts { extern unsigned long long* g_stamp_buf_conv; }
extern "C" int itts_debug_stamps_conv(void* buf) {
#if ITTS_STAMPS
  itts::g_stamp_buf_conv = (unsigned long long*)buf;
  return ITTS_OK;
#else
  (void)buf;
  return ITTS_ERR_INVALID;
#endif
}

// the same for itts_sample: 16 x u64 per batch row (see tools/timeline_sample.py for the stamp positions)
extern "C" int itts_debug_stamps_sample(void* buf) {
#if ITTS_STAMPS
  itts::g_stamp_buf_sample = (unsigned long long*)buf;
  return ITTS_OK;
#else
  (void)buf;
  return ITTS_ERR_INVALID;
#endif
}
#endif
