// libindextts_pitch.so (include/indextts_pitch.h): resampling of a ragged batch by a ratio per row for gfx950 -- the second step
// of the pitch shift, behind WSOLA at speed / p (indextts/utils/tempo.py).  One kernel; the header
// states the computation.
//
// resample_ratio: grid (tiles, rows); one workgroup (4 waves, 256 threads) owns ITTR_TILE = 1024 consecutive outputs of ONE row.
//   It stages in LDS the table (3076 floats, 16-byte loads) and the span of the row its outputs read: at most
//   (TILE - 1) p + 2 H <= 2070 samples for p <= 2, H <= 12, through the 16-byte groups of the aligned span around them (a row
//   starts on a 16-byte boundary; a sample outside the row is zero, a group across a row's end is read sample by sample).
//   20 624 bytes of LDS: seven workgroups, 28 waves, a CU.  Thread t computes the outputs m0 + t + 256 q, q < 4: neighbouring
//   lanes read the span p words apart (two lanes a bank at p = 2) and the table wherever their phases fall; their stores are
//   one 256-byte run a wave.  A lane sums its 2 H taps in rising order; positions and table indices are integers throughout.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_pitch.h"

namespace ittr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int HW = ITTR_HW, PH = ITTR_PHASES;
constexpr int WG = 256;                              // threads of a workgroup
constexpr int PER = ITTR_TILE / WG;                  // outputs per thread
constexpr int H_MAX = (HW * ITTR_CUTOFF_ONE + ITTR_CUTOFF_MIN - 1) / ITTR_CUTOFF_MIN;
constexpr int SPAN = 2080;                           // floats of a tile's span in LDS
constexpr int64_t MAX_N = (int64_t)1 << 30;
static_assert(PH == 256 && ITTR_TABLE == 2 * HW * PH + 4 && ITTR_TABLE % 4 == 0, "k = U >> 24 indexes PH = 2^8 phases a tap; the table is closed by zeros");
static_assert(H_MAX == 12 && ITTR_STEP_MAX == (2ull << 32), "the span bound below is for p <= 2 and H <= 12");
static_assert((ITTR_TILE - 1) * 2 + 2 * H_MAX + 3 <= SPAN && SPAN % 4 == 0, "a tile's span, from the 16-byte boundary below it, fits");
static_assert(PER * WG == ITTR_TILE, "whole rounds of the workgroup");
static_assert(sizeof(ittr_row) == 48, "table layout of the header");

__host__ __device__ inline int taps_a_side(uint32_t cutoff) { return (int)(((uint32_t)HW * ITTR_CUTOFF_ONE + cutoff - 1) / cutoff); }

// Why a row is refused (0: it is taken).  The entry point runs this on the host copy of the table and the kernel on the device
// copy: one statement of the range checks.
__host__ __device__ inline int row_refusal(const ittr_row& r, int64_t x_elems, int64_t y_elems) {
  if (r.n < 1 || r.n >= MAX_N || r.n_out < 1 || r.n_out >= MAX_N) return 1;
  if (r.step < ITTR_STEP_MIN || r.step > ITTR_STEP_MAX) return 2;
  if (r.cutoff < ITTR_CUTOFF_MIN || r.cutoff > ITTR_CUTOFF_ONE) return 3;
  if ((r.x_off & 3) != 0 || (r.y_off & 3) != 0) return 4;
  if (r.x_off < 0 || r.x_off > x_elems || r.n > x_elems - r.x_off) return 5;
  if (r.y_off < 0 || r.y_off > y_elems || r.n_out > y_elems - r.y_off) return 6;
  return 0;
}

struct RatioParams {
  const float* x;
  float* y;
  const float* table;
  const ittr_row* rows;
  int64_t x_elems, y_elems;
};

__global__ void __launch_bounds__(WG) resample_ratio(RatioParams p) {
  __shared__ __attribute__((aligned(16))) float s_g[ITTR_TABLE];
  __shared__ __attribute__((aligned(16))) float s_x[SPAN];
  const int tid = threadIdx.x;
  const ittr_row row = p.rows[blockIdx.y];
  // what the host checked on its copy of the table, again on the one this launch reads
  if (row_refusal(row, p.x_elems, p.y_elems)) return;
  const int64_t n = row.n, n_out = row.n_out;
  const int64_t m0 = (int64_t)blockIdx.x * ITTR_TILE;        // this workgroup's outputs are m0 .. m1
  if (m0 >= n_out) return;
  const int64_t m1 = (m0 + ITTR_TILE < n_out ? m0 + ITTR_TILE : n_out) - 1;
  const uint64_t step = row.step;
  const int64_t cutoff = row.cutoff;
  const int H = taps_a_side(row.cutoff);
  // m step < 2^30 2^33: no overflow.  The taps of m0 .. m1 lie in [lo, hi]; the span is staged from the 16-byte boundary g0 below
  const int64_t lo = (int64_t)(((uint64_t)m0 * step) >> 32) - H + 1;
  const int64_t hi = (int64_t)(((uint64_t)m1 * step) >> 32) + H;
  const int64_t g0 = lo & ~(int64_t)3;
  const int groups = (int)((hi - g0) / 4) + 1;
  if (groups > SPAN / 4) return;                             // (not reached: step and cutoff are in their ranges)
  for (int q = tid; q < ITTR_TABLE / 4; q += WG)
    reinterpret_cast<f32x4*>(s_g)[q] = reinterpret_cast<const f32x4*>(p.table)[q];
  const float* x = p.x + row.x_off;                          // the row's first sample: on a 16-byte boundary
  for (int q = tid; q < groups; q += WG) {
    const int64_t g = g0 + 4 * (int64_t)q;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g >= 0 && g + 3 < n) {
      v = *reinterpret_cast<const f32x4*>(x + g);
    } else if (g + 3 >= 0 && g < n) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (g + e >= 0 && g + e < n) v[e] = x[g + e];
    }
    reinterpret_cast<f32x4*>(s_x)[q] = v;
  }
  __syncthreads();
  const float gain = (float)row.cutoff * (1.0f / ITTR_CUTOFF_ONE);   // exact: 17 bits, a power of two
  const int64_t dec = cutoff << 16;
  const int64_t top = (int64_t)(2 * HW) << 32;
  float* y = p.y + row.y_off;
#pragma unroll 1
  for (int q = 0; q < PER; ++q) {
    const int64_t m = m0 + tid + WG * q;
    if (m > m1) break;
    const uint64_t pos = (uint64_t)m * step;
    const int64_t i0 = (int64_t)(pos >> 32);
    const int64_t f = (int64_t)(pos & 0xffffffffull);
    const float* xs = s_x + (int)(i0 - H + 1 - g0);          // xs[j] = xz[i0 - H + 1 + j], 0 <= j < 2 H: inside [lo, hi]
    int64_t U = (((f + ((int64_t)(H - 1) << 32)) * cutoff) >> 16) + ((int64_t)HW << 32);
    float acc = 0.f;
    for (int j = 0; j < 2 * H; ++j, U -= dec) {
      const bool in = U >= 0 && U < top;
      const int k = in ? (int)(U >> 24) : 0;
      const float t = (float)(int)(U & 0xffffff) * (1.0f / 16777216.0f);
      const float ga = s_g[k], gb = s_g[k + 1];
      const float w = in ? fmaf(t, gb - ga, ga) : 0.f;
      acc = fmaf(w, xs[j], acc);
    }
    y[m] = acc * gain;
  }
}

}  // namespace ittr

#define ITTR_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittr::set_error(__VA_ARGS__);  \
      return ITTR_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

extern "C" int ittr_abi_version(void) { return ITTR_ABI_VERSION; }
extern "C" const char* ittr_last_error(void) { return ittr::g_err; }

extern "C" int ittr_resample_ratio(const ittr_resample_ratio_args* a, void* stream) {
  using namespace ittr;
  const char* who = "ittr_resample_ratio";
  ITTR_REQUIRE(a != nullptr, "%s: null argument struct", who);
  ITTR_REQUIRE(a->x && a->y && a->table && a->rows && a->rows_dev, "%s: null pointer", who);
  ITTR_REQUIRE(aligned(a->x, 16) && aligned(a->table, 16) && aligned(a->y, 4) && aligned(a->rows_dev, 8),
               "%s: x and table must be 16-byte aligned, rows_dev 8-byte aligned, y 4-byte aligned", who);
  ITTR_REQUIRE(a->n_rows >= 1 && a->n_rows <= 65535, "%s: n_rows must be 1..65535 (got %d)", who, a->n_rows);
  ITTR_REQUIRE(a->x_elems >= 0 && a->y_elems >= 0, "%s: negative element count", who);
  {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(a->x), x1 = x0 + 4 * (uintptr_t)a->x_elems;
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(a->y), y1 = y0 + 4 * (uintptr_t)a->y_elems;
    ITTR_REQUIRE(!(x0 < y1 && y0 < x1), "%s: y overlaps x (an output would be read as another output's input)", who);
  }
  int64_t most = 0;
  for (int r = 0; r < a->n_rows; ++r) {
    const ittr_row& g = a->rows[r];
    switch (row_refusal(g, a->x_elems, a->y_elems)) {
      case 0: break;
      case 1: ITTR_REQUIRE(false, "%s: row %d has n = %lld samples and n_out = %lld outputs (1 <= n, n_out < 2^30)", who, r, (long long)g.n, (long long)g.n_out);
      case 2: ITTR_REQUIRE(false, "%s: row %d has the step %llu (p in 32.32 fixed point, %llu <= step <= %llu)", who, r, (unsigned long long)g.step,
                           (unsigned long long)ITTR_STEP_MIN, (unsigned long long)ITTR_STEP_MAX);
      case 3: ITTR_REQUIRE(false, "%s: row %d has the cutoff %u (c in units of 2^-16, %d <= cutoff <= %d)", who, r, g.cutoff, ITTR_CUTOFF_MIN, ITTR_CUTOFF_ONE);
      case 4: ITTR_REQUIRE(false, "%s: row %d has an offset that is no multiple of 4 (x_off = %lld, y_off = %lld)", who, r, (long long)g.x_off, (long long)g.y_off);
      case 5: ITTR_REQUIRE(false, "%s: row %d lies outside x (x_off = %lld, n = %lld, x_elems = %lld)", who, r, (long long)g.x_off, (long long)g.n, (long long)a->x_elems);
      default: ITTR_REQUIRE(false, "%s: row %d has n_out = %lld outputs: y too small (y_off = %lld, y_elems = %lld)", who, r, (long long)g.n_out, (long long)g.y_off,
                            (long long)a->y_elems);
    }
    if (g.n_out > most) most = g.n_out;
  }
  RatioParams p;
  p.x = a->x, p.y = a->y, p.table = a->table, p.rows = a->rows_dev;
  p.x_elems = a->x_elems, p.y_elems = a->y_elems;
  dim3 grid((unsigned)((most + ITTR_TILE - 1) / ITTR_TILE), a->n_rows);      // (most < 2^30: at most 2^20 tiles)
  hipLaunchKernelGGL(resample_ratio, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", who, hipGetErrorString(e));
    return ITTR_ERR_LAUNCH;
  }
  return ITTR_OK;
}
