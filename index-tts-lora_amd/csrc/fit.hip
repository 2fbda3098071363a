// libindextts_fit.so (include/indextts_fit.h): voice fitting for gfx950 -- the LoRA factor gradient and the optimizer of
// IndexTTS.fit_voice (indextts/gpt/fit.py).  Five kernels; the header states the quantities and the order of
// every sum.
//
// wgrad: a tall-skinny reduction over the rows on the matrix pipe.  G^T-tile = s^T z: the A operand is s read down its columns
//   (row j of the 16 x 16 product is factor row j, k is the batch row m), the B operand z (k = m, column c).  A wave owns 16 columns
//   of z and every 16-row tile of the rank (at most 4 accumulators), a workgroup of 4 waves 64 columns, over ONE chunk of
//   ITTF_CHUNK rows: z is read once, s once per 16 columns (r <= 64 values a row: it stays in cache).  The operands go from memory
//   to the registers as the instruction wants them -- there is no reuse inside a wave that LDS could serve.  The 16-bit form reads a
//   lane's 8 consecutive rows of one column with 8 two-byte loads (16 lanes: 32 contiguous bytes each): it is priced by those
//   requests, not by the matrix pipe (DESIGN.md section 4.29 names the staged form as a follow-up).
// merge: a thread per (j, c) adds the chunks' partial sums in rising order.
// sqnorm_slices / sqnorm_final, adamw: a workgroup per slice of ITTF_SLICE elements of the table's concatenated segments.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_fit.h"

namespace ittf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int WG = 256;
constexpr int MAX_C = 1 << 24, MAX_LD = MAX_C + 64;
constexpr int MAX_JT = ITTF_MAX_RANK / 16;
static_assert(ITTF_CHUNK % 32 == 0, "a chunk is whole matrix steps of either type");
static_assert(ITTF_SLICE % WG == 0, "a thread of a slice takes the same number of elements");
static_assert(sizeof(ittf_segment) == 64, "the table's records are 64 bytes");

template <class T>
struct Half;
template <>
struct Half<__bf16> {
  typedef bf16x8 frag;
  static __device__ inline f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct Half<_Float16> {
  typedef f16x8 frag;
  static __device__ inline f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct WgradParams {
  const void* s;
  const void* z;
  float* G;
  float* ws;                                         // [n_chunks][16 JT][C]
  int64_t M;
  int r, C, lds, ldz, ldg;
  int JT, CG;                                        // 16-row tiles of the rank; groups of 64 columns
  int n_chunks, accumulate;
  float scale;
};

template <class T>
__global__ void __launch_bounds__(WG) wgrad(WgradParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, cl = lane & 15;
  const int64_t q = blockIdx.x / p.CG;
  const int c0 = ((int)(blockIdx.x % p.CG) * 4 + wave) * 16;
  if (c0 >= p.C) return;                             // (the whole wave: nothing below meets another wave)
  const int c = c0 + cl;
  const bool col = c < p.C;
  const int64_t m_lo = q * ITTF_CHUNK, m_hi = p.M - m_lo < ITTF_CHUNK ? p.M : m_lo + ITTF_CHUNK;
  const T* s = static_cast<const T*>(p.s);
  const T* z = static_cast<const T*>(p.z);
  f32x4 acc[MAX_JT];
#pragma unroll
  for (int jt = 0; jt < MAX_JT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (sizeof(T) == 4) {
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += 4) {    // lane l: A[row j = l & 15][k = l >> 4], B[k = l >> 4][column l & 15]
      const int64_t m = m0 + g;
      const bool live = m < m_hi;                    // a row past the chunk -- past M in the last one -- is never read
      const float b = live && col ? z[m * p.ldz + c] : 0.f;
#pragma unroll
      for (int jt = 0; jt < MAX_JT; ++jt)
        if (jt < p.JT) {
          const int j = jt * 16 + cl;
          const float a = live && j < p.r ? s[m * p.lds + j] : 0.f;
          acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[jt], 0, 0, 0);
        }
    }
  } else {
    typedef typename Half<T>::frag frag;
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += 32) {   // lane l: k = 8 (l >> 4) .. + 7 of row | column l & 15
      const int64_t mb = m0 + 8 * g;
      frag b;
#pragma unroll
      for (int i = 0; i < 8; ++i) b[i] = mb + i < m_hi && col ? z[(mb + i) * p.ldz + c] : (T)0.f;
#pragma unroll
      for (int jt = 0; jt < MAX_JT; ++jt)
        if (jt < p.JT) {
          const int j = jt * 16 + cl;
          frag a;
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = mb + i < m_hi && j < p.r ? s[(mb + i) * p.lds + j] : (T)0.f;
          acc[jt] = Half<T>::mma(a, b, acc[jt]);
        }
    }
  }
  // the product's element (row j, column c) is register j & 3 of lane 16 (j >> 2) + c
  if (!col) return;
#pragma unroll
  for (int jt = 0; jt < MAX_JT; ++jt)
    if (jt < p.JT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = jt * 16 + g * 4 + e;           // (rows r .. 16 JT - 1 of a partial sum are zeros: inside ws all the same)
        p.ws[(q * (16 * p.JT) + j) * p.C + c] = acc[jt][e];
      }
    }
}

__global__ void __launch_bounds__(WG) merge(WgradParams p) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= (int64_t)p.r * p.C) return;
  const int j = (int)(i / p.C), c = (int)(i % p.C);
  float sum = 0.f;
  for (int64_t q = 0; q < p.n_chunks; ++q) sum = __fadd_rn(sum, p.ws[(q * (16 * p.JT) + j) * p.C + c]);   // in rising order
  float v = __fmul_rn(sum, p.scale);
  float* out = p.G + (int64_t)j * p.ldg + c;
  if (p.accumulate) v = __fadd_rn(*out, v);
  *out = v;
}

// the sum of the 256 threads' values (valid in thread 0): t with t + 128, then + 64, ... + 1
__device__ inline float tree(float v, float* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = WG / 2; d >= 1; d >>= 1) {
    if (t < d) sh[t] = __fadd_rn(sh[t], sh[t + d]);
    __syncthreads();
  }
  return sh[0];
}

// f(segment, element index in it) for the elements of slice `slice` that thread t owns -- lo + t, lo + t + 256, ... -- in rising order
template <class F>
__device__ inline void for_slice(const ittf_segment* tab, int n_seg, int64_t total, int64_t slice, F f) {
  const int t = threadIdx.x;
  const int64_t lo = slice * ITTF_SLICE, hi = total - lo < ITTF_SLICE ? total : lo + ITTF_SLICE;
  int first_seg = 0;                                 // the last segment that starts at or before lo: a binary search on start
  for (int hi_seg = n_seg; hi_seg - first_seg > 1;) {
    const int mid = first_seg + (hi_seg - first_seg) / 2;
    if (tab[mid].start <= lo) first_seg = mid; else hi_seg = mid;
  }
  for (int i = first_seg; i < n_seg; ++i) {
    const int64_t st = tab[i].start, n = tab[i].n;
    if (st >= hi) break;                             // (the table is in rising order of start)
    const int64_t a = st > lo ? st : lo, b = st + n < hi ? st + n : hi;
    if (a >= b) continue;
    const int off = (int)(a - lo);                   // the first element >= a of this thread's residue
    const int64_t first = lo + off + ((t - off % WG + WG) % WG);
    for (int64_t idx = first; idx < b; idx += WG) f(tab[i], idx - st);
  }
}

__global__ void __launch_bounds__(WG) sqnorm_slices(const ittf_segment* tab, int n_seg, int64_t total, float* ws) {
  __shared__ float sh[WG];
  float acc = 0.f;
  for_slice(tab, n_seg, total, blockIdx.x, [&](const ittf_segment& sg, int64_t k) {
    const float x = sg.g[k];
    acc = fmaf(x, x, acc);
  });
  const float sum = tree(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(WG) sqnorm_final(const float* ws, int64_t n_slices, float* out) {
  __shared__ float sh[WG];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n_slices; i += WG) acc = __fadd_rn(acc, ws[i]);
  const float sum = tree(acc, sh);
  if (threadIdx.x == 0) out[0] = sum;
}

struct AdamParams {
  const ittf_segment* tab;
  int n_seg;
  int64_t total;
  float decay[2], step[2];                           // 1 - lr wd and lr / bc1 of each group
  float beta1c, beta2, beta2c, eps, bc2_sqrt, clip;  // beta1c = 1 - beta1, beta2c = 1 - beta2
};

template <class T>
__global__ void __launch_bounds__(WG) adamw(AdamParams a) {
  for_slice(a.tab, a.n_seg, a.total, blockIdx.x, [&](const ittf_segment& sg, int64_t k) {
    const int G = sg.group & 1;
    const float g = __fmul_rn(a.clip, sg.g[k]);
    float p = __fmul_rn(sg.p[k], a.decay[G]);
    float m = sg.m[k];
    m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), a.beta1c));
    const float v = fmaf(__fmul_rn(g, a.beta2c), g, __fmul_rn(sg.v[k], a.beta2));
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);
    p = __fsub_rn(p, __fmul_rn(a.step[G], __fdiv_rn(m, denom)));
    sg.p[k] = p, sg.m[k] = m, sg.v[k] = v;
    if (sg.t_copy) static_cast<T*>(sg.t_copy)[k] = (T)p;
  });
}

}  // namespace ittf

#define ITTF_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittf::set_error(__VA_ARGS__);  \
      return ITTF_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

static bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (uintptr_t)a_bytes;
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (uintptr_t)b_bytes;
  return a0 < b1 && b0 < a1;
}

static int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ittf::set_error("%s: %s", who, hipGetErrorString(e));
    return ITTF_ERR_LAUNCH;
  }
  return ITTF_OK;
}

static bool dtype_ok(int d) { return d == ITTF_F32 || d == ITTF_BF16 || d == ITTF_F16; }

extern "C" int ittf_abi_version(void) { return ITTF_ABI_VERSION; }
extern "C" const char* ittf_last_error(void) { return ittf::g_err; }

extern "C" int64_t ittf_wgrad_ws_bytes(int64_t M, int r, int C) {
  if (M < 1 || M >= ((int64_t)1 << 31) - ITTF_CHUNK || r < 1 || r > ITTF_MAX_RANK || C < 1 || C > ittf::MAX_C) return 0;
  return 4 * ((M + ITTF_CHUNK - 1) / ITTF_CHUNK) * (16 * ((r + 15) / 16)) * (int64_t)C;
}

extern "C" int ittf_lora_wgrad(const ittf_lora_wgrad_args* a, void* stream) {
  using namespace ittf;
  ITTF_REQUIRE(a != nullptr, "ittf_lora_wgrad: null argument struct");
  ITTF_REQUIRE(a->s && a->z && a->G && a->ws, "ittf_lora_wgrad: null pointer (s, z, G, ws)");
  ITTF_REQUIRE(dtype_ok(a->dtype), "ittf_lora_wgrad: dtype = %d (ITTF_F32, ITTF_BF16 or ITTF_F16)", a->dtype);
  const int esz = a->dtype == ITTF_F32 ? 4 : 2;
  ITTF_REQUIRE(aligned(a->s, esz) && aligned(a->z, esz) && aligned(a->G, 4) && aligned(a->ws, 16),
               "ittf_lora_wgrad: s and z must be aligned to their element, G to 4 bytes, ws to 16 bytes");
  ITTF_REQUIRE(a->M >= 1 && a->M < ((int64_t)1 << 31) - ITTF_CHUNK, "ittf_lora_wgrad: M must be in [1, 2^31 - %d) (got %lld)", ITTF_CHUNK,
               (long long)a->M);
  ITTF_REQUIRE(a->r >= 1 && a->r <= ITTF_MAX_RANK, "ittf_lora_wgrad: r = %d (1 .. %d)", a->r, ITTF_MAX_RANK);
  ITTF_REQUIRE(a->C >= 1 && a->C <= MAX_C, "ittf_lora_wgrad: C = %d (1 .. 2^24)", a->C);
  ITTF_REQUIRE(a->lds >= a->r && a->lds <= MAX_LD, "ittf_lora_wgrad: lds = %d (the pitch of s: >= r = %d)", a->lds, a->r);
  ITTF_REQUIRE(a->ldz >= a->C && a->ldz <= MAX_LD, "ittf_lora_wgrad: ldz = %d (the pitch of z: >= C = %d)", a->ldz, a->C);
  ITTF_REQUIRE(a->ldg >= a->C && a->ldg <= MAX_LD, "ittf_lora_wgrad: ldg = %d (the pitch of G: >= C = %d)", a->ldg, a->C);
  const int64_t need = ittf_wgrad_ws_bytes(a->M, a->r, a->C);
  ITTF_REQUIRE(a->ws_bytes >= need, "ittf_lora_wgrad: ws too small (%lld bytes, %lld rows of rank %d over %d columns need %lld)",
               (long long)a->ws_bytes, (long long)a->M, a->r, a->C, (long long)need);
  WgradParams p;
  p.s = a->s, p.z = a->z, p.G = a->G, p.ws = static_cast<float*>(a->ws);
  p.M = a->M, p.r = a->r, p.C = a->C, p.lds = a->lds, p.ldz = a->ldz, p.ldg = a->ldg;
  p.JT = (a->r + 15) / 16, p.CG = (a->C + 63) / 64;
  const int64_t n_chunks = (a->M + ITTF_CHUNK - 1) / ITTF_CHUNK;
  p.n_chunks = (int)n_chunks, p.accumulate = a->accumulate != 0, p.scale = a->scale;
  ITTF_REQUIRE(n_chunks * p.CG < ((int64_t)1 << 31), "ittf_lora_wgrad: %lld chunks of %d column groups are too many workgroups",
               (long long)n_chunks, p.CG);
  const int64_t g_bytes = 4 * ((int64_t)(a->r - 1) * a->ldg + a->C);
  const int64_t s_bytes = esz * ((a->M - 1) * a->lds + a->r), z_bytes = esz * ((a->M - 1) * a->ldz + a->C);
  ITTF_REQUIRE(!overlap(a->G, g_bytes, a->s, s_bytes) && !overlap(a->G, g_bytes, a->z, z_bytes), "ittf_lora_wgrad: G overlaps s or z");
  ITTF_REQUIRE(!overlap(a->ws, need, a->s, s_bytes) && !overlap(a->ws, need, a->z, z_bytes) && !overlap(a->ws, need, a->G, g_bytes),
               "ittf_lora_wgrad: ws overlaps s, z or G");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(n_chunks * p.CG));
  if (a->dtype == ITTF_F32) hipLaunchKernelGGL(wgrad<float>, grid, dim3(WG), 0, st, p);
  else if (a->dtype == ITTF_BF16) hipLaunchKernelGGL(wgrad<__bf16>, grid, dim3(WG), 0, st, p);
  else hipLaunchKernelGGL(wgrad<_Float16>, grid, dim3(WG), 0, st, p);
  if (int rc = launched("ittf_lora_wgrad")) return rc;
  hipLaunchKernelGGL(merge, dim3((unsigned)(((int64_t)a->r * a->C + WG - 1) / WG)), dim3(WG), 0, st, p);
  return launched("ittf_lora_wgrad");
}

extern "C" int64_t ittf_sqnorm_ws_floats(int64_t total) {
  if (total < 1 || total >= ((int64_t)1 << 40)) return 0;
  return (total + ITTF_SLICE - 1) / ITTF_SLICE;
}

static int check_table(const char* who, const ittf_segment* table, int n_seg, int64_t total) {
  ITTF_REQUIRE(table != nullptr, "%s: null segment table", who);
  ITTF_REQUIRE(aligned(table, 16), "%s: the segment table must be 16-byte aligned", who);
  ITTF_REQUIRE(n_seg >= 1 && n_seg <= 65536, "%s: n_seg = %d (1 .. 65536)", who, n_seg);
  ITTF_REQUIRE(total >= 1 && total < ((int64_t)1 << 40), "%s: total = %lld elements (1 .. 2^40 - 1)", who, (long long)total);
  return ITTF_OK;
}

extern "C" int ittf_sqnorm(const ittf_segment* table, int n_seg, int64_t total, float* ws, int64_t ws_floats, float* out, void* stream) {
  using namespace ittf;
  if (int rc = check_table("ittf_sqnorm", table, n_seg, total)) return rc;
  ITTF_REQUIRE(ws && out, "ittf_sqnorm: null pointer (ws, out)");
  ITTF_REQUIRE(aligned(ws, 4) && aligned(out, 4), "ittf_sqnorm: ws and out must be 4-byte aligned");
  const int64_t n_slices = ittf_sqnorm_ws_floats(total);
  ITTF_REQUIRE(ws_floats >= n_slices, "ittf_sqnorm: ws too small (%lld floats, %lld elements need %lld)", (long long)ws_floats,
               (long long)total, (long long)n_slices);
  ITTF_REQUIRE(!overlap(out, 4, ws, 4 * n_slices), "ittf_sqnorm: out overlaps ws");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sqnorm_slices, dim3((unsigned)n_slices), dim3(WG), 0, st, table, n_seg, total, ws);
  if (int rc = launched("ittf_sqnorm")) return rc;
  hipLaunchKernelGGL(sqnorm_final, dim3(1), dim3(WG), 0, st, ws, n_slices, out);
  return launched("ittf_sqnorm");
}

extern "C" int ittf_adamw_step(const ittf_adamw_args* a, void* stream) {
  using namespace ittf;
  ITTF_REQUIRE(a != nullptr, "ittf_adamw_step: null argument struct");
  if (int rc = check_table("ittf_adamw_step", a->table, a->n_seg, a->total)) return rc;
  ITTF_REQUIRE(dtype_ok(a->dtype), "ittf_adamw_step: dtype = %d (ITTF_F32, ITTF_BF16 or ITTF_F16)", a->dtype);
  ITTF_REQUIRE(a->beta1 >= 0. && a->beta1 < 1. && a->beta2 >= 0. && a->beta2 < 1., "ittf_adamw_step: beta1 = %g, beta2 = %g (in [0, 1))",
               a->beta1, a->beta2);
  ITTF_REQUIRE(a->eps > 0., "ittf_adamw_step: eps = %g (> 0)", a->eps);
  ITTF_REQUIRE(a->bc1 > 0. && a->bc1 <= 1. && a->bc2_sqrt > 0. && a->bc2_sqrt <= 1.,
               "ittf_adamw_step: bias corrections bc1 = %g, bc2_sqrt = %g (in (0, 1])", a->bc1, a->bc2_sqrt);
  ITTF_REQUIRE(a->clip >= 0. && a->clip <= 1., "ittf_adamw_step: clip = %g (in [0, 1])", a->clip);
  for (int G = 0; G < 2; ++G)
    ITTF_REQUIRE(a->lr[G] >= 0. && a->wd[G] >= 0. && a->lr[G] * a->wd[G] < 1., "ittf_adamw_step: group %d: lr = %g, wd = %g (>= 0, lr wd < 1)", G,
                 a->lr[G], a->wd[G]);
  AdamParams p;
  p.tab = a->table, p.n_seg = a->n_seg, p.total = a->total;
  for (int G = 0; G < 2; ++G) p.decay[G] = (float)(1. - a->lr[G] * a->wd[G]), p.step[G] = (float)(a->lr[G] / a->bc1);
  p.beta1c = (float)(1. - a->beta1), p.beta2 = (float)a->beta2, p.beta2c = (float)(1. - a->beta2);
  p.eps = (float)a->eps, p.bc2_sqrt = (float)a->bc2_sqrt, p.clip = (float)a->clip;
  const dim3 grid((unsigned)ittf_sqnorm_ws_floats(a->total));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->dtype == ITTF_F32) hipLaunchKernelGGL(adamw<float>, grid, dim3(WG), 0, st, p);
  else if (a->dtype == ITTF_BF16) hipLaunchKernelGGL(adamw<__bf16>, grid, dim3(WG), 0, st, p);
  else hipLaunchKernelGGL(adamw<_Float16>, grid, dim3(WG), 0, st, p);
  return launched("ittf_adamw_step");
}
