// FP8 (E4M3) weight-only forms of the skinny GEMM: itts_gemm_skinny_w8, its planner and the weight packer
// (include/indextts_hip.h).  The kernel is gemm_skinny_kernel<..., W8 = true> of gemm_skinny_kernel.h: the decode step
// streams one byte per weight, converts the codes to the activation type in registers and runs the 16-bit MFMAs; every
// epilogue is the 16-bit kernel's, behind one multiplication by the column's scale.
#include "gemm_skinny_kernel.h"

namespace itts {

// one thread per 16-byte chunk of the packed image (layout: include/indextts_hip.h)
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

static int skinny_w8_no_form(const SkinnyPlan& q, bool fold) {
  set_error("itts_gemm_skinny_w8: no form <%d,%d,%d,%d> is built", q.MT, q.SPWc, q.ntb, (int)fold);
  return ITTS_ERR_INVALID;
}

// the instantiations that exist for this (T, MT, FOLD): the same list as plan_skinny's register-budget rules over the FP8 walk
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

extern "C" int itts_gemm_skinny_w8(const itts_skinny_args* a, void* stream) {
  int ksplit, y_mtp, kv_bs_log2;
  if (int rc = skinny_check(a, "itts_gemm_skinny_w8", true, &ksplit, &y_mtp, &kv_bs_log2)) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0, rows = 0; r0 < a->M; r0 += rows) {
    const int MTall = skinny_row_tiles(a->dtype, a->M - r0, a->rows_per_wg, &rows);
    const SkinnyParams p = skinny_params_of(a, r0, rows, 2, y_mtp, kv_bs_log2);
    const SkinnyPlan q = plan_skinny(skinny_walk_w8(p.K), p.N, 1, MTall, a->rows_per_wg, false, p.cvec != nullptr);
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
  return skinny_plan_out8(plan_skinny(skinny_walk_w8(K), N, 1, MTall, rows_per_wg, false, fold != 0), out8);
}
