// FP8 (E4M3) weight-only forms of the skinny GEMM: itts_gemm_skinny_w8, its planner and the weight packer
// (include/indextts_hip_w8.h).  The kernel is gemm_skinny_kernel<..., W8 = true> of gemm_skinny_kernel.h: the decode step
// streams one byte per weight, converts the codes to the activation type in registers and runs the 16-bit MFMAs; every
// epilogue is the 16-bit kernel's, behind one multiplication by the column's scale.
#include "gemm_skinny_kernel.h"

namespace itts {

// one thread per 16-byte chunk of the packed image (layout: include/indextts_hip_w8.h)
__global__ void pack_weight_w8_kernel(const uint8_t* __restrict__ codes, uint8_t* __restrict__ out, int K, int N, int NT, int KB) {
  const int64_t chunk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (chunk >= (int64_t)NT * KB * 64) return;
  const int lane = (int)(chunk & 63);
  const int64_t blk = chunk >> 6;
  const int kb = (int)(blk % KB), nt = (int)(blk / KB);
  const int g = lane >> 4, n = nt * 16 + (lane & 15);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = kb * 64 + (e >> 3) * 32 + g * 8 + (e & 7);
    const uint32_t c = (k < K && n < N) ? codes[(int64_t)k * N + n] : 0u;
    w[e >> 2] |= c << (8 * (e & 3));
  }
  B16 v = {{w[0], w[1], w[2], w[3]}};
  *reinterpret_cast<B16*>(out + chunk * 16) = v;
}

// Geometry of one FP8 launch: plan_skinny's rules with the weight BLOCK (64 k) as the unit of the K walk.  A wave keeps 3 or 5
// blocks per pass -- 6 or 10 activation fragments per row tile, the register classes of the 16-bit kernel's 5- and 10-step forms
// with half the weight registers -- so the column-tile limits are those of plan_skinny with 3 in the place of 5 and 5 of 10.
// No split-K, no 16-wave form.
static SkinnyPlan plan_skinny_w8(int N, int K, int MTall, int rows_per_wg, bool fold) {
  SkinnyPlan q;
  int MT = MTall;
  if (rows_per_wg > 0 && rows_per_wg / 16 < MTall) MT = rows_per_wg / 16;
  const int gz = (MTall + MT - 1) / MT;
  const int KT = (K / 32 + 1) / 2;
  const int NW = KT > 8 ? 8 : KT;
  const int spw = (KT + NW - 1) / NW;
  const int NT = (N + 15) / 16;
  int ntb = (NT * gz + 255) / 256;   // keep the grid within one round of the 256 CUs
  const int SPWc = spw <= 3 ? 3 : 5;
  const int ntb_max = (fold && MT <= 2 && SPWc == 3) ? 4 : 3;
  if (ntb > ntb_max) ntb = ntb_max;
  if (SPWc == 5 && ntb > 2) ntb = 2;
  if (MT > 2 && SPWc == 5) ntb = 1;
  if (fold && MT > 2 && ntb > 2) ntb = 2;
  q.NW = NW;
  q.spw = spw;
  q.ntb = ntb;
  q.SPWc = SPWc;
  q.MT = MT;
  q.gx = (NT + ntb - 1) / ntb;
  q.gy = 1;
  q.gz = gz;
  q.lds = (size_t)NW * ntb * MT * 256 * 4 + (fold ? (size_t)NW * MT * 32 * 4 : 0);
  if (q.lds < 1024) q.lds = 1024;
  return q;
}

static int skinny_w8_no_form(const SkinnyPlan& q, bool fold) {
  set_error("itts_gemm_skinny_w8: no form <%d,%d,%d,%d> is built", q.MT, q.SPWc, q.ntb, (int)fold);
  return ITTS_ERR_INVALID;
}

// the instantiations that exist for this (T, MT, FOLD): the same list as plan_skinny_w8's register-budget rules
template <typename T, int MT, bool FOLD>
static int launch_skinny_w8_mt(const SkinnyParams& p, const SkinnyPlan& q, hipStream_t s) {
  dim3 grid(q.gx, q.gy, q.gz), block(q.NW * 64);
#define ITTS_SK8(SPW_, NTB_)                                                                                  \
  if (q.SPWc == SPW_ && q.ntb == NTB_) {                                                                      \
    hipLaunchKernelGGL((gemm_skinny_kernel<T, MT, SPW_, NTB_, FOLD, 8, true>), grid, block, q.lds, s, SKINNY_LEAD_ARGS(p, q), static_cast<const SkinnyTail&>(p));     \
    return check_launch("itts_gemm_skinny_w8");                                                               \
  }
  ITTS_SK8(3, 1)
  ITTS_SK8(3, 2)
  if constexpr (!(FOLD && MT > 2)) ITTS_SK8(3, 3)
  if constexpr (FOLD && MT <= 2) ITTS_SK8(3, 4)
  ITTS_SK8(5, 1)
  if constexpr (MT <= 2) ITTS_SK8(5, 2)
#undef ITTS_SK8
  return skinny_w8_no_form(q, FOLD);
}

template <typename T>
static int launch_skinny_w8(const SkinnyParams& p, const SkinnyPlan& q, hipStream_t s) {
  const bool fold = p.cvec != nullptr;
  switch (q.MT) {
#define ITTS_MT8(MT_) \
  case MT_: return fold ? launch_skinny_w8_mt<T, MT_, true>(p, q, s) : launch_skinny_w8_mt<T, MT_, false>(p, q, s)
    ITTS_MT8(1);
    ITTS_MT8(2);
    ITTS_MT8(4);
    ITTS_MT8(6);
#undef ITTS_MT8
  }
  return skinny_w8_no_form(q, fold);
}

}  // namespace itts

using namespace itts;

extern "C" int64_t itts_packed_bytes_w8(int K, int N) {
  return (int64_t)((N + 15) / 16) * ((K + 63) / 64) * 1024;
}

extern "C" int itts_pack_weight_w8(const void* codes, void* packed, int K, int N, void* stream) {
  ITTS_REQUIRE(codes && packed && K > 0 && N > 0, "itts_pack_weight_w8: bad arguments");
  const int NT = (N + 15) / 16, KB = (K + 63) / 64;
  const int64_t total = (int64_t)NT * KB * 64;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(pack_weight_w8_kernel, grid, block, 0, (hipStream_t)stream, (const uint8_t*)codes, (uint8_t*)packed, K, N, NT, KB);
  return check_launch("itts_pack_weight_w8");
}

extern "C" int itts_gemm_skinny_w8(const itts_skinny_w8_args* a, void* stream) {
  ITTS_REQUIRE(a && a->wp && a->x, "itts_gemm_skinny_w8: null args");
  ITTS_REQUIRE(a->w_scale, "itts_gemm_skinny_w8: w_scale is null");
  ITTS_REQUIRE(a->dtype == ITTS_BF16 || a->dtype == ITTS_F16, "itts_gemm_skinny_w8: the activation type must be bf16 or f16 (dtype %d)",
               a->dtype);
  ITTS_REQUIRE(a->ksplit <= 1, "itts_gemm_skinny_w8: ksplit=%d is not built (the FP8 forms run without split-K)", a->ksplit);
  ITTS_REQUIRE(a->M >= 0 && a->N > 0 && a->K > 0 && a->K % 32 == 0, "itts_gemm_skinny_w8: bad shape M=%d N=%d K=%d (K %% 32 != 0)", a->M,
               a->N, a->K);
  const int kv_bs_log2 = kv_block_log2(a->epi == ITTS_EPI_QKV_CACHE && a->kv_tab != nullptr, a->kv_bs);
  if (a->epi == ITTS_EPI_QKV_CACHE)
    ITTS_REQUIRE(a->y && a->kcache && a->vcache && a->pos && a->N % 3 == 0 && a->N / 3 == a->heads * 64 &&
                     (a->kv_tab != nullptr ? kv_bs_log2 >= 0 : a->smax > 0),
                 "itts_gemm_skinny_w8: bad QKV epilogue arguments (paged cache: kv_bs must be 16, 32 or 64)");
  else if (a->epi == ITTS_EPI_RESID_F32 || a->epi == ITTS_EPI_STORE_F32)
    ITTS_REQUIRE(a->yf, "itts_gemm_skinny_w8: yf is null");
  else
    ITTS_REQUIRE((a->epi == ITTS_EPI_STORE || a->epi == ITTS_EPI_GELU_STORE) && a->y,
                 "itts_gemm_skinny_w8: epilogue %d is not built (STORE, GELU_STORE, RESID_F32, QKV_CACHE, STORE_F32)", a->epi);
  if (a->epi == ITTS_EPI_RESID_F32)
    ITTS_REQUIRE(a->N % 4 == 0 && (int64_t)a->M * a->N < (1ll << 29), "itts_gemm_skinny_w8: the residual epilogue needs N %% 4 == 0");
  if (a->ln_c != nullptr)
    ITTS_REQUIRE(a->bias && a->N % 4 == 0 && a->epi != ITTS_EPI_RESID_F32,
                 "itts_gemm_skinny_w8: the LayerNorm-folded form needs bias (= d), N %% 4 == 0, a storing epilogue");
  ITTS_REQUIRE(a->rows_per_wg == 0 || a->rows_per_wg == 16 || a->rows_per_wg == 32, "itts_gemm_skinny_w8: rows_per_wg must be 0, 16 or 32");
  if (a->y_packed)
    ITTS_REQUIRE((a->epi == ITTS_EPI_STORE || a->epi == ITTS_EPI_GELU_STORE || a->epi == ITTS_EPI_RESID_F32) && a->N % 32 == 0 && a->y,
                 "itts_gemm_skinny_w8: a packed y needs the STORE / GELU_STORE / RESID_F32 epilogue and N %% 32 == 0");
  const int y_mtp = a->y_mtp > 0 ? a->y_mtp : (a->M + 15) / 16;
  ITTS_REQUIRE(a->y_row0 >= 0 && a->y_row0 % 16 == 0 && (!a->y_packed || a->y_row0 + a->M <= y_mtp * 16) &&
                   (a->y_packed || (a->y_row0 == 0 && a->y_mtp == 0)),
               "itts_gemm_skinny_w8: y_row0 / y_mtp place the rows of a PACKED y inside a taller operand (y_row0 %% 16 == 0)");
  ITTS_REQUIRE(a->x_mtp == 0 || (a->x_packed && a->x_mtp * 16 >= a->M), "itts_gemm_skinny_w8: x_mtp is for a packed x of at least M rows");
  if (a->M == 0) return ITTS_OK;
  ITTS_REQUIRE(a->M <= 96 || a->rows_per_wg == 0 || (a->M + 15) / 16 / (a->rows_per_wg / 16) < 65535, "itts_gemm_skinny_w8: too many rows");
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0, rows = 0; r0 < a->M; r0 += rows) {
    const int MTall = skinny_row_tiles(a->dtype, a->M - r0, a->rows_per_wg, &rows);
    SkinnyParams p = skinny_params_of(a, r0, rows, 2, y_mtp, kv_bs_log2);
    p.w_scale = a->w_scale;
    const SkinnyPlan q = plan_skinny_w8(p.N, p.K, MTall, a->rows_per_wg, p.cvec != nullptr);
    const int rc = by_dtype16(a->dtype, "itts_gemm_skinny_w8", [&](auto tag) {
      return launch_skinny_w8<typename decltype(tag)::type>(p, q, s);
    });
    if (rc != ITTS_OK) return rc;
  }
  return ITTS_OK;
}

extern "C" int itts_skinny_plan_w8(int dtype, int M, int N, int K, int rows_per_wg, int fold, int* out8) {
  ITTS_REQUIRE(out8 && N > 0 && K > 0 && K % 32 == 0 && M > 0, "itts_skinny_plan_w8: bad arguments");
  ITTS_REQUIRE(dtype == ITTS_BF16 || dtype == ITTS_F16, "itts_skinny_plan_w8: the activation type must be bf16 or f16 (dtype %d)", dtype);
  int rows;
  const int MTall = skinny_row_tiles(dtype, M, rows_per_wg, &rows);   // (of the first launch, when the rows take several)
  const SkinnyPlan q = plan_skinny_w8(N, K, MTall, rows_per_wg, fold != 0);
  out8[0] = q.gx; out8[1] = q.gy; out8[2] = q.NW; out8[3] = q.ntb; out8[4] = q.spw; out8[5] = (int)q.lds; out8[6] = q.gz; out8[7] = q.MT;
  return ITTS_OK;
}
