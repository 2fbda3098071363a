// Per-row LoRA adapter bank: the "shrink" half, u = s_a (x A_a^T) scattered into the slot of each row's own adapter.
//
// y = x W + s_a (x A_a^T) B_a^T = [x | u] [W ; B_bank^T]: the consuming GEMM (itts_gemm_skinny in the decode step, itts_gemm_conv
// in the large-M passes) runs unchanged over K + K_x, with the K_x extra operand columns written here and the K_x extra weight
// rows holding every adapter's B^T.  The LoRA term thereby lands in the GEMM's fp32 accumulator, in front of the bias, the GELU
// and the K/V append of its epilogue.
//
// Work shape: rows of one 16-row tile generally carry different adapters, so this is a per-row GEMV gather, not a tile GEMM.
// One workgroup of NWV waves per row; the 16-byte pieces of the row's K range are dealt to the lanes (piece p -> wave p / 64 % NWV,
// lane p % 64), every lane keeps rp fp32 accumulators, one per row of A_a.  A 16-row chunk of A_a is requested as 16 coalesced
// 1-KiB wave loads per piece.  Reduction: a transposing butterfly inside the wave (17 cross-lane moves per 16 accumulators instead
// of 96), then the waves' partials through LDS in wave order.  No atomics: the summation order is fixed by the shape alone.
// Traffic per row: rp x K elements of A (40 KB at r = 16, K = 1280 in bf16) -- from L2 once two rows share a voice.
#include "common.h"

namespace itts {

constexpr int LORA_NWV = 4;   // waves per row

struct LoraShrinkParams {
  const void* x;
  const int32_t* ids;
  const void* a_bank;
  void* u;
  int64_t ldu;
  int M, K, n, rp, Kx;
  int x_packed, x_mtp, u_packed, u_mtp;
};

// v[0 .. 16) of every lane -> the wave's sum of v[j], j = (lane >> 2) & 15 read as bits (5 4 3 2) = (8 4 2 1), in every lane of
// the group of four that shares those bits.  Each halving step sends the half a lane does not keep to its partner.
template <int HALF, int OFF>
__device__ __forceinline__ void reduce_half(float (&v)[16], const int lane) {
  const bool up = (lane & OFF) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float send = up ? v[i] : v[i + HALF];
    const float keep = up ? v[i + HALF] : v[i];
    v[i] = keep + __shfl_xor(send, OFF, 64);
  }
}
__device__ __forceinline__ float reduce16(float (&v)[16], const int lane) {
  reduce_half<8, 32>(v, lane);
  reduce_half<4, 16>(v, lane);
  reduce_half<2, 8>(v, lane);
  reduce_half<1, 4>(v, lane);
  float s = v[0];
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  return s;
}

// NCH = rp / 16 chunks of 16 rows of A
template <typename T, int NCH>
__global__ __launch_bounds__(LORA_NWV * 64) void lora_shrink_kernel(LoraShrinkParams p) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = EL::E;
  __shared__ float part[LORA_NWV][NCH * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x;   // < M, or a padding row of the packed tail (written as zeros)
  int a = -1;
  if (m < p.M) a = p.ids[m];
  if (a >= p.n) a = -1;       // (the host checks the ids; an id outside the bank must still not read outside it)
  const T* X = (const T*)p.x;
  const T* A = (const T*)p.a_bank + (int64_t)(a < 0 ? 0 : a) * p.rp * p.K;

  if (a >= 0) {   // block-uniform
    float acc[NCH][16];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[c][j] = 0.f;
    for (int k0 = (wave * 64 + lane) * E; k0 < p.K; k0 += LORA_NWV * 64 * E) {
      const frag xf = ld16<frag>(p.x_packed ? X + pa_off<T>(m, k0, p.x_mtp) : X + (int64_t)m * p.K + k0);
      float xv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xv[e] = EL::to_f(xf[e]);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        frag af[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) af[j] = ld16<frag>(A + (int64_t)(c * 16 + j) * p.K + k0);
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
          for (int e = 0; e < E; ++e) acc[c][j] = fmaf(xv[e], EL::to_f(af[j][e]), acc[c][j]);
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float s = reduce16(acc[c], lane);
      if ((lane & 3) == 0) part[wave][c * 16 + (lane >> 2)] = s;
    }
  }
  __syncthreads();
  // every column of the row's K_x, every call: the own slot from the partials (wave order), zeros everywhere else
  T* U = (T*)p.u;
  const int lo = a * p.rp;
  for (int col0 = tid * E; col0 < p.Kx; col0 += LORA_NWV * 64 * E) {
    frag o;
    const int j0 = col0 - lo;   // rp % 16 == 0 and E | 16: a piece lies inside the slot or outside it
    const bool own = a >= 0 && j0 >= 0 && j0 < p.rp;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float s = 0.f;
      if (own) {
        const int slot = j0 + e;   // reduce16 leaves accumulator j of a chunk in lane group j = lane >> 2
        s = part[0][slot];
#pragma unroll
        for (int w = 1; w < LORA_NWV; ++w) s += part[w][slot];
      }
      o[e] = EL::from_f(s);
    }
    st16(p.u_packed ? U + pa_off<T>(m, col0, p.u_mtp) : U + (int64_t)m * p.ldu + col0, o);
  }
}

template <typename T>
static int launch_lora_shrink(const LoraShrinkParams& p, int rows, hipStream_t s) {
  dim3 grid(rows), block(LORA_NWV * 64);
  switch (p.rp / 16) {
    case 1: hipLaunchKernelGGL((lora_shrink_kernel<T, 1>), grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL((lora_shrink_kernel<T, 2>), grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL((lora_shrink_kernel<T, 3>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((lora_shrink_kernel<T, 4>), grid, block, 0, s, p); break;
  }
  return check_launch("itts_lora_shrink");
}

}  // namespace itts

using namespace itts;

extern "C" int itts_lora_shrink(const itts_lora_shrink_args* a, void* stream) {
  ITTS_REQUIRE(a && a->x && a->ids && a->a_bank && a->u, "itts_lora_shrink: null args");
  return by_dtype(a->dtype, "itts_lora_shrink", [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int ks = Elem<T>::KS, e = Elem<T>::E;
    ITTS_REQUIRE(a->M >= 0 && a->K > 0 && a->K % ks == 0, "itts_lora_shrink: bad shape M=%d K=%d (K %% %d != 0)", a->M, a->K, ks);
    ITTS_REQUIRE(a->n >= 1 && a->rp >= 16 && a->rp <= 64 && a->rp % 16 == 0,
                 "itts_lora_shrink: n=%d adapters of padded rank rp=%d (1 <= n, rank <= 64, rp %% 16 == 0)", a->n, a->rp);
    ITTS_REQUIRE(a->Kx <= 512 && a->Kx == ((int64_t)a->n * a->rp + 31) / 32 * 32,
                 "itts_lora_shrink: Kx=%d must be n * rp rounded up to a multiple of 32, and <= 512", a->Kx);
    const int mtp = (a->M + 15) / 16;
    const int x_mtp = a->x_mtp > 0 ? a->x_mtp : mtp, u_mtp = a->u_mtp > 0 ? a->u_mtp : mtp;
    ITTS_REQUIRE((a->x_packed || a->x_mtp == 0) && x_mtp * 16 >= a->M, "itts_lora_shrink: x_mtp is for a packed x of at least M rows");
    ITTS_REQUIRE((a->u_packed || a->u_mtp == 0) && u_mtp * 16 >= a->M, "itts_lora_shrink: u_mtp is for a packed u of at least M rows");
    ITTS_REQUIRE(a->u_packed || (a->ldu >= a->Kx && a->ldu % e == 0), "itts_lora_shrink: a row-major u needs ldu >= Kx, ldu %% %d == 0", e);
    ITTS_REQUIRE(((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->u & 15) == 0 && ((uintptr_t)a->a_bank & 15) == 0,
                 "itts_lora_shrink: x, u and a_bank must be 16-byte aligned");
    if (a->M == 0) return ITTS_OK;
    LoraShrinkParams p;
    p.x = a->x;
    p.ids = a->ids;
    p.a_bank = a->a_bank;
    p.u = a->u;
    p.ldu = a->ldu;
    p.M = a->M;
    p.K = a->K;
    p.n = a->n;
    p.rp = a->rp;
    p.Kx = a->Kx;
    p.x_packed = a->x_packed ? 1 : 0;
    p.x_mtp = x_mtp;
    p.u_packed = a->u_packed ? 1 : 0;
    p.u_mtp = u_mtp;
    const int rows = p.u_packed ? u_mtp * 16 : a->M;   // the packed tail's padding rows are written too (zeros)
    return launch_lora_shrink<T>(p, rows, (hipStream_t)stream);
  });
}
