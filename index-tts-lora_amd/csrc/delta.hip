// libindextts_voice.so (include/indextts_voice.h): Y = op(D) X with D = float(Wt) - float(Wb) formed in registers, for gfx950.
//
// Voice extraction (indextts/gpt/voice_extract.py) needs products of the difference of two [K][N]
// checkpoints with c-wide fp32 blocks, c <= 80.  The work is one pass over the two weight images: 4 bytes of 16-bit weights per
// c multiply-adds, so the kernel is shaped around the loads -- every lane takes 8 consecutive n of one row k from both images
// with 16-byte non-temporal loads, subtracts in fp32, and feeds the 8 differences to 8 v_mfma_f32_16x16x4_f32 (exact fp32
// fmaf-chain numerics) whose reduction slot is the lane's own; the c-wide operand comes from L1/L2.
//   op = identity (delta_rows):  D is the A operand.  Lane (r, g) holds D[k0 + r][n0 + 8g + j], MFMA j reduces over the four n
//       = n0 + 8g + j, g = 0..3; the B operand of MFMA j is X[n0 + 8g + j][16 ct + r].  One workgroup (one wave): 16 rows k.
//   op = transpose (delta_cols): D is the B operand.  Lane (r, g) holds D[k0 + g][n0 + 8r + j], MFMA j owns the 16 columns
//       n0 + 8r + j and reduces over the four k = k0 + g; the A operand is X[k0 + g][16 ct + r], shared by the 8 MFMAs.  One
//       workgroup: 128 columns n.
// 16 rows (128 columns) times the whole reduction is far too few waves to keep the memory system busy, so the host splits the
// reduction over S workgroups per tile.  Each writes its partial tile to a slab; the one that draws the last ticket of the
// tile's counter (an integer atomic) adds the S slabs in split order 0, 1, .. S-1 and writes Y.  Which workgroup arrives last
// varies from run to run, what it computes does not: no floating-point atomics, the same bits every time.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_voice.h"

namespace ittv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// 8 consecutive elements of a weight image as fp32, through 16-byte loads of bytes this launch reads exactly once
template <int DT>
struct Image;
template <>
struct Image<ITTV_F32> {
  static constexpr const char* name = "f32";
  static __device__ __forceinline__ void load8(const void* base, size_t elem, float (&d)[8]) {
    const u32x4* p = reinterpret_cast<const u32x4*>(static_cast<const float*>(base) + elem);
    u32x4 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = __uint_as_float(a[i]), d[4 + i] = __uint_as_float(b[i]);
  }
};
template <>
struct Image<ITTV_BF16> {
  static constexpr const char* name = "bf16";
  static __device__ __forceinline__ void load8(const void* base, size_t elem, float (&d)[8]) {
    u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + elem));
#pragma unroll
    for (int i = 0; i < 4; ++i) d[2 * i] = __uint_as_float(a[i] << 16), d[2 * i + 1] = __uint_as_float(a[i] & 0xffff0000u);
  }
};
template <>
struct Image<ITTV_F16> {
  static constexpr const char* name = "f16";
  static __device__ __forceinline__ void load8(const void* base, size_t elem, float (&d)[8]) {
    u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + elem));
    f16x8 h = __builtin_bit_cast(f16x8, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (float)h[i];
  }
};

// A workgroup is ONE wave: the kernels keep a tile's accumulators in that wave's registers, and combine() below orders the slab
// stores of all 64 lanes before lane 0's ticket by the wave's own program order -- no barrier, no LDS flag.  A wider workgroup
// would need both (a barrier in front of the release, the "I am last" flag through LDS): WG is what launch bounds and launch use.
constexpr int WG = 64;
static_assert(WG == 64, "delta_rows / delta_cols / combine are written for one-wave workgroups");

struct Params {
  const void* wt;
  const void* wb;
  const float* x;
  float* y;
  float* slab;   // S partial images of y, split s at slab + s * out_elems (S > 1)
  int* cnt;      // one ticket counter per tile, zero at launch (S > 1)
  int K, N;
  int S, chunk;  // the reduction is cut into S pieces of `chunk` (the last one may be shorter)
  int64_t out_elems;
};

// The end of a workgroup of a split reduction: publish the slab, draw a ticket; the last arriver of the tile adds the slabs in
// split order.  Release before the ticket, acquire behind it, both at agent scope (the L2s of the XCDs are not coherent).
__device__ __forceinline__ void combine(const Params& p, int tile, size_t off, int n4) {
  const int lane = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int ticket = 0;
  if (lane == 0) ticket = __hip_atomic_fetch_add(p.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  if (ticket != p.S - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const f32x4* src = reinterpret_cast<const f32x4*>(p.slab + off);
  f32x4* dst = reinterpret_cast<f32x4*>(p.y + off);
  const size_t stride4 = (size_t)p.out_elems / 4;
  for (int i = lane; i < n4; i += WG) {
    f32x4 a = src[i];
    for (int s = 1; s < p.S; ++s) a += src[s * stride4 + i];
    dst[i] = a;
  }
}

// y [K][c] = D x,  x [N][c]:  workgroup (tile, s) owns rows [16 tile, +16) and the n of piece s
template <int DTT, int DTB, int CT>
__global__ void __launch_bounds__(WG) delta_rows(Params p) {
  constexpr int C = 16 * CT;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, s = blockIdx.y;
  const int n_beg = s * p.chunk, n_end = min(p.N, n_beg + p.chunk);
  const size_t row = (size_t)(tile * 16 + r) * p.N;
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n0 = n_beg; n0 < n_end; n0 += 64) {
    float wt[2][8], wb[2][8];
    int nl[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {          // a lane past the end reads the piece's first elements and contributes zeros
      const int n = n0 + 32 * u + 8 * g;
      ok[u] = n < n_end;
      nl[u] = ok[u] ? n : n_beg;
      Image<DTT>::load8(p.wt, row + nl[u], wt[u]);
      Image<DTB>::load8(p.wb, row + nl[u], wb[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float* xr = p.x + (size_t)nl[u] * C + r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = ok[u] ? wt[u][j] - wb[u][j] : 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, xr[j * C + 16 * ct], acc[ct], 0, 0, 0);
      }
    }
  }
  // accumulator register i of lane (r, g): row 4g + i of the tile, column 16 ct + r
  const size_t off = (size_t)tile * 16 * C;
  float* dst = (p.S == 1 ? p.y : p.slab + (size_t)s * p.out_elems) + off;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(4 * g + i) * C + 16 * ct + r] = acc[ct][i];
  if (p.S > 1) combine(p, tile, off, 16 * C / 4);
}

// y [N][c] = D^T x,  x [K][c]:  workgroup (tile, s) owns columns [128 tile, +128) and the k of piece s
template <int DTT, int DTB, int CT>
__global__ void __launch_bounds__(WG) delta_cols(Params p) {
  constexpr int C = 16 * CT;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, s = blockIdx.y;
  const int k_beg = s * p.chunk, k_end = min(p.K, k_beg + p.chunk);   // both multiples of 16
  const int n = tile * 128 + 8 * r;
  const bool ok = n < p.N;                   // N is a multiple of 16: a lane's 8 columns exist together or not at all
  const int nc = ok ? n : 0;
  f32x4 acc[8][CT];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[j][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = k_beg; k0 < k_end; k0 += 16) {
    float wt[4][8], wb[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t e = (size_t)(k0 + 4 * u + g) * p.N + nc;
      Image<DTT>::load8(p.wt, e, wt[u]);
      Image<DTB>::load8(p.wb, e, wb[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* xr = p.x + (size_t)(k0 + 4 * u + g) * C + r;
      float xa[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) xa[ct] = xr[16 * ct];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = ok ? wt[u][j] - wb[u][j] : 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[j][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ct], d, acc[j][ct], 0, 0, 0);
      }
    }
  }
  // accumulator (j, ct), register i of lane (r, g): x column 16 ct + 4g + i of output row n + j
  const size_t off = (size_t)tile * 128 * C;
  const int rows = min(128, p.N - tile * 128);
  float* dst = (p.S == 1 ? p.y : p.slab + (size_t)s * p.out_elems) + off;
  if (ok) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) *reinterpret_cast<f32x4*>(dst + (size_t)(8 * r + j) * C + 16 * ct + 4 * g) = acc[j][ct];
  }
  if (p.S > 1) combine(p, tile, off, rows * C / 4);
}

// The launch plan, a function of the shape alone: tiles, and the split of the reduction that brings the grid to about `target`
// waves (4 resp. 2 per CU of loads in flight) while a piece keeps at least two loop passes and the slabs fit the workspace.
struct Plan {
  int tiles, S, chunk;
};
constexpr int64_t SLAB_BYTES = ITTV_DELTA_WS_BYTES - (64 << 10);
static Plan make_plan(int K, int N, int c, int trans) {
  const int R = trans ? K : N, out_rows = trans ? N : K;
  const int unit = trans ? 16 : 32, target = trans ? 512 : 1024;
  Plan pl;
  pl.tiles = trans ? (N + 127) / 128 : K / 16;
  int S = 1;
  if (pl.tiles < target) {
    S = (target + pl.tiles - 1) / pl.tiles;
    const int max_s = R / (2 * unit);
    if (S > max_s) S = max_s;
    if (S > 64) S = 64;
    const int64_t out_bytes = (int64_t)out_rows * c * 4;
    while (S > 1 && S * out_bytes > SLAB_BYTES) --S;
    if (S < 1) S = 1;
  }
  pl.chunk = ((R + S - 1) / S + unit - 1) / unit * unit;
  pl.S = (R + pl.chunk - 1) / pl.chunk;
  return pl;
}

template <int DTT, int DTB, int CT>
static void launch(const Params& p, const Plan& pl, int trans, hipStream_t st) {
  dim3 grid(pl.tiles, pl.S);
  if (trans)
    hipLaunchKernelGGL((delta_cols<DTT, DTB, CT>), grid, dim3(WG), 0, st, p);
  else
    hipLaunchKernelGGL((delta_rows<DTT, DTB, CT>), grid, dim3(WG), 0, st, p);
}
template <int DTT, int DTB>
static void launch_ct(int ct, const Params& p, const Plan& pl, int trans, hipStream_t st) {
  switch (ct) {
    case 1: return launch<DTT, DTB, 1>(p, pl, trans, st);
    case 2: return launch<DTT, DTB, 2>(p, pl, trans, st);
    case 3: return launch<DTT, DTB, 3>(p, pl, trans, st);
    case 4: return launch<DTT, DTB, 4>(p, pl, trans, st);
    case 5: return launch<DTT, DTB, 5>(p, pl, trans, st);
  }
}
template <int DTT>
static void launch_b(int dtb, int ct, const Params& p, const Plan& pl, int trans, hipStream_t st) {
  switch (dtb) {
    case ITTV_F32: return launch_ct<DTT, ITTV_F32>(ct, p, pl, trans, st);
    case ITTV_BF16: return launch_ct<DTT, ITTV_BF16>(ct, p, pl, trans, st);
    case ITTV_F16: return launch_ct<DTT, ITTV_F16>(ct, p, pl, trans, st);
  }
}

}  // namespace ittv

#define ITTV_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittv::set_error(__VA_ARGS__);  \
      return ITTV_ERR_INVALID;       \
    }                                \
  } while (0)

extern "C" int ittv_abi_version(void) { return ITTV_ABI_VERSION; }
extern "C" const char* ittv_last_error(void) { return ittv::g_err; }

extern "C" int ittv_delta_project(const ittv_delta_args* a, void* stream) {
  using namespace ittv;
  ITTV_REQUIRE(a != nullptr, "ittv_delta_project: null argument struct");
  ITTV_REQUIRE(a->wt && a->wb && a->x && a->y && a->ws, "ittv_delta_project: null pointer");
  auto known = [](int d) { return d == ITTV_F32 || d == ITTV_BF16 || d == ITTV_F16; };
  ITTV_REQUIRE(known(a->dtype_t) && known(a->dtype_b), "ittv_delta_project: unknown dtype (%d, %d)", a->dtype_t, a->dtype_b);
  ITTV_REQUIRE(a->K > 0 && a->N > 0 && a->K % 16 == 0 && a->N % 16 == 0,
               "ittv_delta_project: K and N must be positive multiples of 16 (got K=%d N=%d)", a->K, a->N);
  ITTV_REQUIRE(a->c >= 16 && a->c <= 80 && a->c % 16 == 0, "ittv_delta_project: c must be 16, 32, 48, 64 or 80 (got %d)", a->c);
  ITTV_REQUIRE(a->trans == 0 || a->trans == 1, "ittv_delta_project: trans must be 0 or 1 (got %d)", a->trans);
  ITTV_REQUIRE((int64_t)a->K * a->N < ((int64_t)1 << 40), "ittv_delta_project: K * N too large");
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  ITTV_REQUIRE(al(a->wt) && al(a->wb) && al(a->x) && al(a->y) && al(a->ws), "ittv_delta_project: pointers must be 16-byte aligned");
  ITTV_REQUIRE(a->ws_bytes >= ITTV_DELTA_WS_BYTES, "ittv_delta_project: ws must hold ITTV_DELTA_WS_BYTES = %lld bytes (got %lld)",
               (long long)ITTV_DELTA_WS_BYTES, (long long)a->ws_bytes);
  const Plan pl = make_plan(a->K, a->N, a->c, a->trans);
  ITTV_REQUIRE(pl.S >= 1 && pl.S <= 65535 && (pl.S == 1 || pl.tiles * 4 <= (64 << 10)), "ittv_delta_project: no launch plan");
  Params p;
  p.wt = a->wt, p.wb = a->wb, p.x = a->x, p.y = a->y;
  p.cnt = static_cast<int*>(a->ws);
  p.slab = reinterpret_cast<float*>(static_cast<char*>(a->ws) + (64 << 10));
  p.K = a->K, p.N = a->N, p.S = pl.S, p.chunk = pl.chunk;
  p.out_elems = (int64_t)(a->trans ? a->N : a->K) * a->c;
  ITTV_REQUIRE(pl.S == 1 || pl.S * p.out_elems * 4 <= SLAB_BYTES, "ittv_delta_project: the slabs do not fit the workspace");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pl.S > 1 && hipMemsetAsync(p.cnt, 0, (size_t)pl.tiles * 4, st) != hipSuccess) {
    set_error("ittv_delta_project: hipMemsetAsync: %s", hipGetErrorString(hipGetLastError()));
    return ITTV_ERR_LAUNCH;
  }
  switch (a->dtype_t) {
    case ITTV_F32: launch_b<ITTV_F32>(a->dtype_b, a->c / 16, p, pl, a->trans, st); break;
    case ITTV_BF16: launch_b<ITTV_BF16>(a->dtype_b, a->c / 16, p, pl, a->trans, st); break;
    case ITTV_F16: launch_b<ITTV_F16>(a->dtype_b, a->c / 16, p, pl, a->trans, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("ittv_delta_project: %s", hipGetErrorString(e));
    return ITTV_ERR_LAUNCH;
  }
  return ITTV_OK;
}
