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

// ---------------------------------------------------------------------------------------------------------------
// The same launch over weighted MIXES of bank voices (itts_lora_shrink_mix, include/indextts_hip.h): a row names up to four
// adapters, the slot of entry j gets w_j s_{a_j} (x A_{a_j}^T).  lora_shrink_kernel's shape with a wave-uniform loop over the
// record's entries around its K loop: per entry the same pieces, the same rp accumulators, the same butterfly, the same partials
// in wave order -- so a record {a, 1.0f} gives lora_shrink_kernel's bits for id a (w * s is one fp32 multiply in front of the one
// rounding to T, exact at 1.0f), and the order of the entries moves no bit (an entry's partials meet nobody else's).
// A lane's x pieces are its own in every entry.  Its first piece is requested in the kernel's first lines, beside the row's record
// (two 16-byte words of one address for the whole workgroup: the compiler makes them one scalar request), and stays in registers:
// one trip for x and the record, then the A requests.  The first entry fetches the lane's later pieces and keeps LORA_MIX_XT of them
// (K <= 18432 in the 16-bit types, 9216 in fp32) in LDS slots private to the lane -- no barrier -- for the entries that follow;
// pieces of a longer row are requested again (L2 hits).  K = 1280 in bf16 is one piece per lane: no LDS traffic at all.
// Leading arguments: what the first requests need, for the kernarg preload; the output's description trails.
constexpr int LORA_MIX_XT = 8;

template <typename T, int NCH>
__global__ __launch_bounds__(LORA_NWV * 64) void lora_shrink_mix_kernel(const void* x, const itts_lora_mix_row* mix, const void* a_bank,
                                                                        int M, int K, int n, int rp, int x_packed, int x_mtp, void* u,
                                                                        int Kx, int u_packed, int u_mtp, int64_t ldu) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = EL::E, NE = ITTS_LORA_MIX_ENTRIES;
  __shared__ float part[NE][LORA_NWV][NCH * 16];
  __shared__ B16 xs[LORA_MIX_XT][LORA_NWV * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x;   // < M, or a padding row of the packed tail (written as zeros)
  const T* X = (const T*)x;
  // the lane's first piece of x and the row's record are requested together, in front of the first wait: one trip for both
  const int kf = (wave * 64 + lane) * E;
  frag x0 = zero_frag<frag>();
  if (m < M && kf < K) x0 = ld16<frag>(x_packed ? X + pa_off<T>(m, kf, x_mtp) : X + (int64_t)m * K + kf);
  int id[NE];
  float wt[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) id[j] = -1, wt[j] = 0.f;
  if (m < M) {   // block-uniform; the record is the same 32 bytes for every lane
    const u32x4 r0 = ld16<u32x4>(mix + m), r1 = ld16<u32x4>((const char*)(mix + m) + 16);
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const u32x4 r = j < 2 ? r0 : r1;
      id[j] = __builtin_amdgcn_readfirstlane((int)r[(j & 1) * 2]);
      wt[j] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(r[(j & 1) * 2 + 1]));
      if (id[j] >= n) id[j] = -1;   // (the host checks the ids; an id outside the bank must still not read outside it)
    }
  }
  bool have_x = false;   // a lane's later pieces are in xs[] once one entry has gone over the row

#pragma unroll
  for (int j = 0; j < NE; ++j) {
    if (id[j] < 0) continue;   // wave-uniform
    const T* A = (const T*)a_bank + (int64_t)id[j] * rp * K;
    float acc[NCH][16];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
    int t = 0;
    for (int k0 = (wave * 64 + lane) * E; k0 < K; k0 += LORA_NWV * 64 * E, ++t) {
      frag xf = x0;
      if (t > 0) {
        if (have_x && t <= LORA_MIX_XT) {
          xf = ld16<frag>(&xs[t - 1][tid]);
        } else {
          xf = ld16<frag>(x_packed ? X + pa_off<T>(m, k0, x_mtp) : X + (int64_t)m * K + k0);
          if (!have_x && t <= LORA_MIX_XT) st16(&xs[t - 1][tid], xf);
        }
      }
      float xv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xv[e] = EL::to_f(xf[e]);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        frag af[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) af[i] = ld16<frag>(A + (int64_t)(c * 16 + i) * K + k0);
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
          for (int e = 0; e < E; ++e) acc[c][i] = fmaf(xv[e], EL::to_f(af[i][e]), acc[c][i]);
      }
    }
    have_x = true;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float s = reduce16(acc[c], lane);
      if ((lane & 3) == 0) part[j][wave][c * 16 + (lane >> 2)] = s;
    }
  }
  __syncthreads();
  // every column of the row's K_x, every call: the named slots from their entry's partials (wave order) times its weight, zeros
  // everywhere else
  T* U = (T*)u;
  for (int col0 = tid * E; col0 < Kx; col0 += LORA_NWV * 64 * E) {
    int own = -1, j0 = 0;   // rp % 16 == 0 and E | 16: a piece lies inside one slot or outside all
    float w = 0.f;
#pragma unroll
    for (int j = NE - 1; j >= 0; --j) {
      const int d = col0 - id[j] * rp;
      if (id[j] >= 0 && d >= 0 && d < rp) own = j, j0 = d, w = wt[j];
    }
    frag o;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float s = 0.f;
      if (own >= 0) {
        const int slot = j0 + e;   // reduce16 leaves accumulator i of a chunk in lane group i = lane >> 2
        s = part[own][0][slot];
#pragma unroll
        for (int wv = 1; wv < LORA_NWV; ++wv) s += part[own][wv][slot];
        s *= w;
      }
      o[e] = EL::from_f(s);
    }
    st16(u_packed ? U + pa_off<T>(m, col0, u_mtp) : U + (int64_t)m * ldu + col0, o);
  }
}

template <typename T>
static int launch_lora_shrink_mix(const itts_lora_shrink_args& a, int x_mtp, int u_mtp, hipStream_t s) {
  const int rows = a.u_packed ? u_mtp * 16 : a.M;   // the packed tail's padding rows are written too (zeros)
  dim3 grid(rows), block(LORA_NWV * 64);
#define ITTS_MIX_LAUNCH(NCH)                                                                                                       \
  hipLaunchKernelGGL((lora_shrink_mix_kernel<T, NCH>), grid, block, 0, s, a.x, a.mix, a.a_bank, a.M, a.K, a.n, a.rp, a.x_packed ? 1 : 0, \
                     x_mtp, a.u, a.Kx, a.u_packed ? 1 : 0, u_mtp, a.ldu)
  switch (a.rp / 16) {
    case 1: ITTS_MIX_LAUNCH(1); break;
    case 2: ITTS_MIX_LAUNCH(2); break;
    case 3: ITTS_MIX_LAUNCH(3); break;
    default: ITTS_MIX_LAUNCH(4); break;
  }
#undef ITTS_MIX_LAUNCH
  return check_launch("itts_lora_shrink_mix");
}

}  // namespace itts

using namespace itts;

// The checks itts_lora_shrink and itts_lora_shrink_mix share (`who` in every message), after the entry point's own null check; the
// mix adds only the alignment of its records.  Out: the row tiles of a packed x / u.
template <typename T>
static int lora_shrink_check(const itts_lora_shrink_args* a, const char* who, bool mix, int* x_mtp_out, int* u_mtp_out) {
  constexpr int ks = Elem<T>::KS, e = Elem<T>::E;
  ITTS_REQUIRE(a->M >= 0 && a->K > 0 && a->K % ks == 0, "%s: bad shape M=%d K=%d (K %% %d != 0)", who, a->M, a->K, ks);
  ITTS_REQUIRE(a->n >= 1 && a->rp >= 16 && a->rp <= 64 && a->rp % 16 == 0,
               "%s: n=%d adapters of padded rank rp=%d (1 <= n, rank <= 64, rp %% 16 == 0)", who, a->n, a->rp);
  ITTS_REQUIRE(a->Kx <= 512 && a->Kx == ((int64_t)a->n * a->rp + 31) / 32 * 32,
               "%s: Kx=%d must be n * rp rounded up to a multiple of 32, and <= 512", who, a->Kx);
  const int mtp = (a->M + 15) / 16;
  const int x_mtp = a->x_mtp > 0 ? a->x_mtp : mtp, u_mtp = a->u_mtp > 0 ? a->u_mtp : mtp;
  ITTS_REQUIRE((a->x_packed || a->x_mtp == 0) && x_mtp * 16 >= a->M, "%s: x_mtp is for a packed x of at least M rows", who);
  ITTS_REQUIRE((a->u_packed || a->u_mtp == 0) && u_mtp * 16 >= a->M, "%s: u_mtp is for a packed u of at least M rows", who);
  ITTS_REQUIRE(a->u_packed || (a->ldu >= a->Kx && a->ldu % e == 0), "%s: a row-major u needs ldu >= Kx, ldu %% %d == 0", who, e);
  ITTS_REQUIRE(((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->u & 15) == 0 && ((uintptr_t)a->a_bank & 15) == 0 &&
                   (!mix || ((uintptr_t)a->mix & 15) == 0),
               mix ? "%s: x, u, a_bank and mix must be 16-byte aligned" : "%s: x, u and a_bank must be 16-byte aligned", who);
  *x_mtp_out = x_mtp;
  *u_mtp_out = u_mtp;
  return ITTS_OK;
}

extern "C" int itts_lora_shrink(const itts_lora_shrink_args* a, void* stream) {
  ITTS_REQUIRE(a && a->x && a->ids && a->a_bank && a->u, "itts_lora_shrink: null args");
  return by_dtype(a->dtype, "itts_lora_shrink", [&](auto tag) {
    using T = typename decltype(tag)::type;
    int x_mtp, u_mtp;
    if (int rc = lora_shrink_check<T>(a, "itts_lora_shrink", false, &x_mtp, &u_mtp)) return rc;
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

extern "C" int itts_lora_shrink_mix(const itts_lora_shrink_args* a, void* stream) {
  ITTS_REQUIRE(a && a->x && a->mix && a->a_bank && a->u, "itts_lora_shrink_mix: null args");
  return by_dtype(a->dtype, "itts_lora_shrink_mix", [&](auto tag) {
    using T = typename decltype(tag)::type;
    int x_mtp, u_mtp;
    if (int rc = lora_shrink_check<T>(a, "itts_lora_shrink_mix", true, &x_mtp, &u_mtp)) return rc;
    if (a->M == 0) return ITTS_OK;
    return launch_lora_shrink_mix<T>(*a, x_mtp, u_mtp, (hipStream_t)stream);
  });
}
