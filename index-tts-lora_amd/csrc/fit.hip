// libindextts_fit.so (include/indextts_fit.h): voice fitting for gfx950 -- the LoRA factor gradient and the optimizer of
// IndexTTS.fit_voice (indextts/gpt/fit.py), and at the end of the file the four kernels of the ragged causal
// training attention.  The header states the quantities and the order of every sum.
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

// ------------------------------------------------------------------------------------------------ the training attention
// Ragged causal attention for the fit, forward and backward (the header states the quantities and the order of every sum).  A
// wave owns one 16-row tile of one (segment, head) and nothing is shared between waves: a workgroup is one wave, there is no LDS
// and no barrier.  Lane l = 16 g + r.  Every product is a 16 x 16 x 4 fp32 matrix instruction whose operands come from memory as
// float4s: a reduction index may be permuted freely as long as both operands agree, so
//   - a product over the 64 head columns reads, per row r, the columns 16 a + 4 g .. + 3 (a = 0 .. 3): instruction (a, b) sums the
//     columns 16 a + 4 g' + b over g';
//   - a product over a tile's 16 rows reads row 4 g + b with the columns 4 r .. + 3 (b = 0 .. 3): instruction b sums the rows
//     4 g' + b, and output tile c holds the columns 4 rho + c of output row index rho -- register e of lane (r, g) is column
//     16 g + 4 e + c: a lane ends with 16 consecutive columns of row r.
// The scores are computed with the reduction row of the NEXT product on the accumulator's row index (4 g + b), so that an
// accumulator is that product's B operand as it stands: keys in the forward and in dq (S^T = K Q^T), queries in dk / dv (S = Q K^T).
namespace ittf {

struct AttnParams {
  const float* qkv;
  float* out;
  float* lse;
  const float* dout;
  float* dqkv;
  float* delta;                                      // [H][M], the backward's workspace: attn_dq writes it, attn_dkdv reads it
  const ittf_rows* tab;
  int64_t M;
  int max_len, H, ld, ldo;
  float scale;
};

// the rows of segment z, cut at max_len rows and at row M: -> the row count (0: nothing to do), `first` its first row
__device__ inline int attn_segment(const AttnParams& p, int z, int64_t& first) {
  const ittf_rows s = p.tab[z];
  first = s.first;
  if (s.first < 0 || s.first >= p.M || s.count < 1) return 0;
  int64_t n = s.count < p.max_len ? s.count : p.max_len;
  if (n > p.M - s.first) n = p.M - s.first;
  return (int)n;
}

__device__ inline f32x4 ld4(const float* q, bool live) {   // (a row that is not the segment's is never read)
  return live ? *reinterpret_cast<const f32x4*>(q) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ inline f32x4 mma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc += sum over the 64 columns of x[row][.] y[row'][.]: the chain of 16
__device__ inline f32x4 dot64(const f32x4 (&x)[4], const f32x4 (&y)[4], f32x4 acc) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc = mma4(x[a][b], y[a][b], acc);
  return acc;
}

// a lane's 16 consecutive columns 16 g .. 16 g + 15 of its row, times f
__device__ inline void store16(float* dst, const f32x4 (&acc)[4], float f) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    *reinterpret_cast<f32x4*>(dst + 4 * e) =
        f32x4{__fmul_rn(acc[0][e], f), __fmul_rn(acc[1][e], f), __fmul_rn(acc[2][e], f), __fmul_rn(acc[3][e], f)};
}

__global__ void __launch_bounds__(64) attn_fwd(AttnParams p) {
  const int r = threadIdx.x & 15, g = threadIdx.x >> 4, h = blockIdx.y;
  int64_t first;
  const int n = attn_segment(p, blockIdx.z, first);
  const int nt = (n + 15) >> 4;
  if ((int)blockIdx.x >= nt) return;
  const int qt = nt - 1 - (int)blockIdx.x;           // the longest sweeps start first
  const int D = 64 * p.H, qi = qt * 16 + r;
  const bool qlive = qi < n;
  const float* base = p.qkv + first * p.ld + 64 * h;
  f32x4 Q[4], O[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    Q[a] = ld4(base + (int64_t)qi * p.ld + 16 * a + 4 * g, qlive);
    O[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    const int kj = kt * 16 + r;
    f32x4 K[4], V[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) K[a] = ld4(base + D + (int64_t)kj * p.ld + 16 * a + 4 * g, kj < n);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int vj = kt * 16 + 4 * g + b;
      V[b] = ld4(base + 2 * D + (int64_t)vj * p.ld + 4 * r, vj < n);
    }
    const f32x4 S = dot64(K, Q, f32x4{0.f, 0.f, 0.f, 0.f});   // register b: key 4 g + b, query r
    float s[4], tmax = -INFINITY;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      s[b] = kt * 16 + 4 * g + b <= qi ? __fmul_rn(p.scale, S[b]) : -INFINITY;
      tmax = fmaxf(tmax, s[b]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);                 // finite from tile 0 on: key 0 is at or below every query
    const float alpha = expf(__fsub_rn(m, mn));
    float pr[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) pr[b] = expf(__fsub_rn(s[b], mn));
    float t = __fadd_rn(__fadd_rn(__fadd_rn(pr[0], pr[1]), pr[2]), pr[3]);
    t = __fadd_rn(t, __shfl_xor(t, 16));
    t = __fadd_rn(t, __shfl_xor(t, 32));
    l = fmaf(l, alpha, t);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) O[c][e] = __fmul_rn(O[c][e], alpha);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) O[c] = mma4(V[b][c], pr[b], O[c]);   // O^T = V^T P^T: column 4 rho + c of query r
    m = mn;
  }
  if (!qlive) return;
  float* o = p.out + (first + qi) * p.ldo + 64 * h + 16 * g;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    *reinterpret_cast<f32x4*>(o + 4 * e) =
        f32x4{__fdiv_rn(O[0][e], l), __fdiv_rn(O[1][e], l), __fdiv_rn(O[2][e], l), __fdiv_rn(O[3][e], l)};
  if (g == 0) p.lse[(int64_t)h * p.M + first + qi] = __fadd_rn(m, logf(l));
}

__global__ void __launch_bounds__(64) attn_dkdv(AttnParams p) {
  const int r = threadIdx.x & 15, g = threadIdx.x >> 4, h = blockIdx.y;
  int64_t first;
  const int n = attn_segment(p, blockIdx.z, first);
  const int nt = (n + 15) >> 4, kt = blockIdx.x;     // (key tile 0 sweeps the most query tiles and starts first)
  if (kt >= nt) return;
  const int D = 64 * p.H, kj = kt * 16 + r;
  const bool klive = kj < n;
  const float* base = p.qkv + first * p.ld + 64 * h;
  const float* dob = p.dout + first * p.ldo + 64 * h;
  const float* lse = p.lse + (int64_t)h * p.M + first;
  const float* delta = p.delta + (int64_t)h * p.M + first;
  f32x4 K[4], V[4], dK[4], dV[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    K[a] = ld4(base + D + (int64_t)kj * p.ld + 16 * a + 4 * g, klive);
    V[a] = ld4(base + 2 * D + (int64_t)kj * p.ld + 16 * a + 4 * g, klive);
    dK[a] = dV[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int qt = kt; qt < nt; ++qt) {
    const int qi = qt * 16 + r;
    f32x4 Qa[4], Oa[4], Qc[4], Oc[4];
    float ls[4], dl[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      Qa[a] = ld4(base + (int64_t)qi * p.ld + 16 * a + 4 * g, qi < n);
      Oa[a] = ld4(dob + (int64_t)qi * p.ldo + 16 * a + 4 * g, qi < n);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int qb = qt * 16 + 4 * g + b;
      const bool live = qb < n;
      Qc[b] = ld4(base + (int64_t)qb * p.ld + 4 * r, live);
      Oc[b] = ld4(dob + (int64_t)qb * p.ldo + 4 * r, live);
      ls[b] = live ? lse[qb] : 0.f;
      dl[b] = live ? delta[qb] : 0.f;
    }
    const f32x4 S = dot64(Qa, K, f32x4{0.f, 0.f, 0.f, 0.f});   // register b: query 4 g + b, key r
    const f32x4 dP = dot64(Oa, V, f32x4{0.f, 0.f, 0.f, 0.f});
    float pr[4], ds[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int qb = qt * 16 + 4 * g + b;
      pr[b] = kj <= qb && qb < n ? expf(__fsub_rn(__fmul_rn(p.scale, S[b]), ls[b])) : 0.f;
      ds[b] = __fmul_rn(pr[b], __fsub_rn(dP[b], dl[b]));
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dV[c] = mma4(Oc[b][c], pr[b], dV[c]);        // dV^T = dO^T P
        dK[c] = mma4(Qc[b][c], ds[b], dK[c]);        // dK^T = Q^T dS
      }
  }
  if (!klive) return;
  float* dst = p.dqkv + (first + kj) * p.ld + 64 * h + 16 * g;
  store16(dst + D, dK, p.scale);
  store16(dst + 2 * D, dV, 1.f);
}

__global__ void __launch_bounds__(64) attn_dq(AttnParams p) {
  const int r = threadIdx.x & 15, g = threadIdx.x >> 4, h = blockIdx.y;
  int64_t first;
  const int n = attn_segment(p, blockIdx.z, first);
  const int nt = (n + 15) >> 4;
  if ((int)blockIdx.x >= nt) return;
  const int qt = nt - 1 - (int)blockIdx.x;
  const int D = 64 * p.H, qi = qt * 16 + r;
  const bool qlive = qi < n;
  const float* base = p.qkv + first * p.ld + 64 * h;
  const float* dob = p.dout + first * p.ldo + 64 * h;
  f32x4 Q[4], dO[4], dQ[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    Q[a] = ld4(base + (int64_t)qi * p.ld + 16 * a + 4 * g, qlive);
    dO[a] = ld4(dob + (int64_t)qi * p.ldo + 16 * a + 4 * g, qlive);
    dQ[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float ls = qlive ? p.lse[(int64_t)h * p.M + first + qi] : 0.f;
  // the first sweep: delta = sum over the keys of p dP, with the bits of p and dP that the second sweep (and dk / dv) form again
  float delta = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    const int kj = kt * 16 + r;
    f32x4 Ka[4], Va[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      Ka[a] = ld4(base + D + (int64_t)kj * p.ld + 16 * a + 4 * g, kj < n);
      Va[a] = ld4(base + 2 * D + (int64_t)kj * p.ld + 16 * a + 4 * g, kj < n);
    }
    const f32x4 S = dot64(Ka, Q, f32x4{0.f, 0.f, 0.f, 0.f});
    const f32x4 dP = dot64(Va, dO, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float pr = qlive && kt * 16 + 4 * g + b <= qi ? expf(__fsub_rn(__fmul_rn(p.scale, S[b]), ls)) : 0.f;
      delta = fmaf(pr, dP[b], delta);
    }
  }
  delta = __fadd_rn(delta, __shfl_xor(delta, 16));
  delta = __fadd_rn(delta, __shfl_xor(delta, 32));
  if (qlive && g == 0) p.delta[(int64_t)h * p.M + first + qi] = delta;   // for the dk / dv launch behind this one
  for (int kt = 0; kt <= qt; ++kt) {
    const int kj = kt * 16 + r;
    f32x4 Ka[4], Va[4], Kc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      Ka[a] = ld4(base + D + (int64_t)kj * p.ld + 16 * a + 4 * g, kj < n);
      Va[a] = ld4(base + 2 * D + (int64_t)kj * p.ld + 16 * a + 4 * g, kj < n);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int kb = kt * 16 + 4 * g + b;
      Kc[b] = ld4(base + D + (int64_t)kb * p.ld + 4 * r, kb < n);
    }
    const f32x4 S = dot64(Ka, Q, f32x4{0.f, 0.f, 0.f, 0.f});   // register b: key 4 g + b, query r
    const f32x4 dP = dot64(Va, dO, f32x4{0.f, 0.f, 0.f, 0.f});
    float ds[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float pr = qlive && kt * 16 + 4 * g + b <= qi ? expf(__fsub_rn(__fmul_rn(p.scale, S[b]), ls)) : 0.f;
      ds[b] = __fmul_rn(pr, __fsub_rn(dP[b], delta));
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) dQ[c] = mma4(Kc[b][c], ds[b], dQ[c]);   // dQ^T = K^T dS^T
  }
  if (!qlive) return;
  store16(p.dqkv + (first + qi) * p.ld + 64 * h + 16 * g, dQ, p.scale);
}

}  // namespace ittf

extern "C" int64_t ittf_attn_ws_bytes(int64_t M, int H) {
  if (M < 1 || M >= ((int64_t)1 << 31) || H < 1 || H > ITTF_ATTN_MAX_HEADS) return 0;
  return 4 * M * (int64_t)H;
}

static int attn_check(const char* who, const ittf_attn_args* a, bool bwd) {
  using namespace ittf;
  ITTF_REQUIRE(a != nullptr, "%s: null argument struct", who);
  ITTF_REQUIRE(a->qkv && (bwd || a->out) && a->lse && a->table, "%s: null pointer (qkv, out, lse, table)", who);   // (bwd does not read out)
  ITTF_REQUIRE(!bwd || (a->dout && a->dqkv && a->ws), "%s: null pointer (dout, dqkv, ws)", who);
  ITTF_REQUIRE(a->H >= 1 && a->H <= ITTF_ATTN_MAX_HEADS, "%s: H = %d (1 .. %d heads of 64 columns)", who, a->H, ITTF_ATTN_MAX_HEADS);
  const int D = 64 * a->H;
  ITTF_REQUIRE(a->M >= 1 && a->M < ((int64_t)1 << 31), "%s: M must be in [1, 2^31) (got %lld)", who, (long long)a->M);
  ITTF_REQUIRE(a->n_seg >= 1 && a->n_seg <= ITTF_ATTN_MAX_NSEG, "%s: n_seg = %d (1 .. %d)", who, a->n_seg, ITTF_ATTN_MAX_NSEG);
  ITTF_REQUIRE(a->max_len >= 1 && a->max_len <= ITTF_ATTN_MAX_SEG, "%s: max_len = %d: a segment has 1 .. %d rows", who, a->max_len,
               ITTF_ATTN_MAX_SEG);
  ITTF_REQUIRE(a->ld >= 3 * D && a->ld <= MAX_LD && a->ld % 4 == 0, "%s: ld = %d (the pitch of qkv: >= 3 D = %d, a multiple of 4)", who,
               a->ld, 3 * D);
  ITTF_REQUIRE(a->ldo >= D && a->ldo <= MAX_LD && a->ldo % 4 == 0, "%s: ldo = %d (the pitch of out: >= D = %d, a multiple of 4)", who,
               a->ldo, D);
  ITTF_REQUIRE(a->scale > 0.f && a->scale <= 3.0e38f, "%s: scale = %g (finite and > 0)", who, (double)a->scale);
  ITTF_REQUIRE(aligned(a->qkv, 16) && (bwd || aligned(a->out, 16)) && aligned(a->lse, 4) && aligned(a->table, 16),
               "%s: qkv, out and the table must be 16-byte aligned, lse 4-byte aligned", who);
  ITTF_REQUIRE(!bwd || (aligned(a->dout, 16) && aligned(a->dqkv, 16) && aligned(a->ws, 4)),
               "%s: dout and dqkv must be 16-byte aligned, ws 4-byte aligned", who);
  const int64_t qkv_b = 4 * ((a->M - 1) * a->ld + 3 * D), out_b = 4 * ((a->M - 1) * a->ldo + D), lse_b = 4 * a->M * a->H;
  const int64_t tab_b = 16 * (int64_t)a->n_seg;
  if (!bwd) {
    ITTF_REQUIRE(!overlap(a->out, out_b, a->qkv, qkv_b) && !overlap(a->out, out_b, a->table, tab_b) &&
                     !overlap(a->lse, lse_b, a->qkv, qkv_b) && !overlap(a->lse, lse_b, a->table, tab_b) &&
                     !overlap(a->out, out_b, a->lse, lse_b),
                 "%s: out or lse overlaps qkv, the table or the other", who);
    return ITTF_OK;
  }
  const int64_t need = ittf_attn_ws_bytes(a->M, a->H);
  ITTF_REQUIRE(a->ws_bytes >= need, "%s: ws too small (%lld bytes, %lld rows of %d heads need %lld)", who, (long long)a->ws_bytes,
               (long long)a->M, a->H, (long long)need);
  const void* in[4] = {a->qkv, a->lse, a->dout, a->table};
  const int64_t in_b[4] = {qkv_b, lse_b, out_b, tab_b};
  for (int i = 0; i < 4; ++i)
    ITTF_REQUIRE(!overlap(a->dqkv, qkv_b, in[i], in_b[i]) && !overlap(a->ws, need, in[i], in_b[i]),
                 "%s: dqkv or ws overlaps qkv, lse, dout or the table", who);
  ITTF_REQUIRE(!overlap(a->dqkv, qkv_b, a->ws, need), "%s: dqkv overlaps ws", who);
  return ITTF_OK;
}

static ittf::AttnParams attn_params(const ittf_attn_args* a) {
  ittf::AttnParams p;
  p.qkv = a->qkv, p.out = a->out, p.lse = a->lse, p.dout = a->dout, p.dqkv = a->dqkv, p.delta = static_cast<float*>(a->ws);
  p.tab = a->table, p.M = a->M, p.max_len = a->max_len, p.H = a->H, p.ld = a->ld, p.ldo = a->ldo, p.scale = a->scale;
  return p;
}

extern "C" int ittf_attn_fwd(const ittf_attn_args* a, void* stream) {
  using namespace ittf;
  if (int rc = attn_check("ittf_attn_fwd", a, false)) return rc;
  const AttnParams p = attn_params(a);
  const dim3 grid((unsigned)((a->max_len + 15) / 16), (unsigned)a->H, (unsigned)a->n_seg);
  hipLaunchKernelGGL(attn_fwd, grid, dim3(64), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittf_attn_fwd");
}

extern "C" int ittf_attn_bwd(const ittf_attn_args* a, void* stream) {
  using namespace ittf;
  if (int rc = attn_check("ittf_attn_bwd", a, true)) return rc;
  const AttnParams p = attn_params(a);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((a->max_len + 15) / 16), (unsigned)a->H, (unsigned)a->n_seg);
  hipLaunchKernelGGL(attn_dq, grid, dim3(64), 0, st, p);          // (writes delta into ws ...)
  if (int rc = launched("ittf_attn_bwd")) return rc;
  hipLaunchKernelGGL(attn_dkdv, grid, dim3(64), 0, st, p);        // (... which this one reads)
  return launched("ittf_attn_bwd");
}
