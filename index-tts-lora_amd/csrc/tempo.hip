// libindextts_tempo.so (include/indextts_tempo.h): the speaking rate for gfx950 between the vocoder's fp32 samples and waveform
// finishing -- WSOLA time-scale modification at 24 kHz (indextts/utils/tempo.py).  Two kernels; the
// header states the algorithm.
//
// search: grid (rows); ONE workgroup (6 waves, 384 threads) walks a row's chain of lags, a thread one lag.  Per frame the
//   workgroup stages the template (768 floats) and the searched span x[a_k - TOL, a_k + TOL + WIN) (1152 floats) in LDS: 16-byte
//   global loads from the aligned span around them (a row starts on a 16-byte boundary), a sample outside the row is zero.  The
//   inner loop reads the template as one 16-byte broadcast per four terms (every lane the same address) and the span at stride 1
//   across the lanes (lane l of a wave reads word base + l: no two lanes share a bank).  Four partial sums per lag in a fixed
//   order, see the header.  The argmax is a butterfly over the wave (the key orders the score, then the smaller |d|, then the
//   negative lag: a total order, so the butterfly's pairing does not matter), one LDS step over the six waves' winners, and
//   every thread reads the six and knows the frame's lag -- it is where the next frame's template starts.  Two barriers a frame.
//   This kernel's parallelism is bounded by the batch: one CU per row, whatever the row's length.
// overlap_add: grid (runs, rows); one workgroup owns ITTM_RUN = 1024 consecutive outputs of ONE row, a thread four of them (HOP
//   is a multiple of 4: the four lie in one frame).  The two lags of the frame come from `offsets`, the window's eight weights as
//   two 16-byte loads, the samples one by one (their addresses have any alignment); one 16-byte store per thread, the row's
//   last, partial group sample by sample.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_tempo.h"

namespace ittm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int HOP = ITTM_HOP, WIN = ITTM_WIN, TOL = ITTM_TOL;
constexpr int LAGS = 2 * TOL;                        // threads of a search workgroup: one per lag
constexpr int WAVES = LAGS / 64;
constexpr int SPAN = WIN + LAGS;                     // samples a frame's lags read: x[a_k - TOL, a_k + TOL + WIN)
constexpr int OWG = 256;                             // threads of an overlap_add workgroup
constexpr int PER = ITTM_RUN / OWG;                  // outputs per thread
constexpr int64_t MAX_INDEX = (int64_t)1 << 40;
static_assert(LAGS == 384 && WAVES * 64 == LAGS, "one lag per thread, whole waves");
static_assert(WIN % 4 == 0 && SPAN % 4 == 0 && HOP % 4 == 0 && WIN == 2 * HOP, "16-byte groups; the window is two hops");
static_assert(SPAN / 4 + 1 <= LAGS && WIN / 4 + 1 <= LAGS, "a thread stages at most one 16-byte group of each buffer");
static_assert(PER == 4, "a thread assembles four samples per store");
static_assert(sizeof(ittm_row) == 40, "table layout of the header");

__host__ __device__ inline int64_t out_len(int64_t n, int64_t S) {
  const int64_t m = (n * 1024 + S / 2) / S;
  return m < 1 ? 1 : m;
}
__host__ __device__ inline int64_t frames_of(int64_t n_out) { return (n_out - 1) / HOP + 2; }
__host__ __device__ inline int64_t nominal(int64_t k, int64_t S) { return (k * HOP * S + 512) / 1024 - HOP; }

// Why a row is refused (0: it is taken).  The entry points run this on the host copy of the table and the kernels on the device
// copy: one statement of the range checks.  y_elems < 0: the launch has no y (search).
__host__ __device__ inline int row_refusal(const ittm_row& r, int64_t x_elems, int64_t offsets_elems, int64_t y_elems) {
  if (r.n < 1 || r.n >= MAX_INDEX) return 1;
  if (r.speed < ITTM_SPEED_MIN || r.speed > ITTM_SPEED_MAX) return 2;
  if (r.x_off < 0 || r.x_off >= MAX_INDEX || r.x_off + r.n > x_elems) return 3;
  if ((r.x_off & 3) != 0 || (r.o_off & 3) != 0 || (y_elems >= 0 && (r.y_off & 3) != 0)) return 4;
  const int64_t n_out = out_len(r.n, r.speed);
  if (r.o_off < 0 || r.o_off >= MAX_INDEX || r.o_off + frames_of(n_out) > offsets_elems) return 5;
  if (y_elems >= 0 && (r.y_off < 0 || r.y_off >= MAX_INDEX || r.y_off + n_out > y_elems)) return 6;
  return 0;
}

// dst[j] = xz[start + j] for j < len (a multiple of 4), through the 16-byte groups of the aligned span around them: thread q of
// the first len / 4 + 1 loads the group at (start rounded down to a multiple of 4) + 4 q -- x is the row's first sample, on a
// 16-byte boundary -- and puts its samples where they belong.
__device__ inline void stage(float* dst, int len, const float* x, int64_t n, int64_t start, int tid) {
  if (tid > len / 4) return;
  const int64_t g0 = start & ~(int64_t)3;
  const int sh = (int)(start - g0);
  const int64_t g = g0 + 4 * (int64_t)tid;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (g >= 0 && g + 3 < n) {
    v = *reinterpret_cast<const f32x4*>(x + g);
  } else if (g + 3 >= 0 && g < n) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (g + e >= 0 && g + e < n) v[e] = x[g + e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * tid + e - sh;
    if (j >= 0 && j < len) dst[j] = v[e];
  }
}

// is the lag d1 of score c1 chosen before d2 of c2?  the larger score; of equal scores the smaller |d|; of +-d the negative one
__device__ inline bool before(float c1, int d1, float c2, int d2) {
  if (c1 != c2) return c1 > c2;
  const int m1 = d1 < 0 ? -d1 : d1, m2 = d2 < 0 ? -d2 : d2;
  return m1 != m2 ? m1 < m2 : d1 < d2;
}

struct SearchParams {
  const float* x;
  int32_t* offsets;
  const ittm_row* rows;
  int64_t x_elems, offsets_elems;
};

__global__ void __launch_bounds__(LAGS) search(SearchParams p) {
  __shared__ __attribute__((aligned(16))) float s_tpl[WIN];
  __shared__ __attribute__((aligned(16))) float s_span[SPAN];
  __shared__ float s_c[WAVES];
  __shared__ int s_d[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const ittm_row row = p.rows[blockIdx.x];
  // what the host checked on its copy of the table, again on the one this launch reads
  if (row_refusal(row, p.x_elems, p.offsets_elems, -1)) return;
  const int64_t S = row.speed, n = row.n;
  const int64_t K = frames_of(out_len(n, S));
  const float* x = p.x + row.x_off;
  int32_t* off = p.offsets + row.o_off;
  if (tid == 0) off[0] = 0;
  int64_t prev = -HOP;                                       // p_(k-1)
  for (int64_t k = 1; k < K; ++k) {
    const int64_t a = nominal(k, S);
    stage(s_tpl, WIN, x, n, prev + HOP, tid);
    stage(s_span, SPAN, x, n, a - TOL, tid);
    __syncthreads();
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const float* w = s_span + tid;                           // lag d = tid - TOL reads xz[a + d + i] = span[tid + i]
#pragma unroll 8
    for (int i = 0; i < WIN; i += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(s_tpl + i);
      s0 = fmaf(t[0], w[i], s0);
      s1 = fmaf(t[1], w[i + 1], s1);
      s2 = fmaf(t[2], w[i + 2], s2);
      s3 = fmaf(t[3], w[i + 3], s3);
    }
    float c = (s0 + s1) + (s2 + s3);
    int d = tid - TOL;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float oc = __shfl_xor(c, m, 64);
      const int od = __shfl_xor(d, m, 64);
      if (before(oc, od, c, d)) c = oc, d = od;
    }
    if (lane == 0) s_c[wave] = c, s_d[wave] = d;
    __syncthreads();                                         // (also: every thread is done with s_tpl and s_span)
    c = s_c[0], d = s_d[0];
#pragma unroll
    for (int v = 1; v < WAVES; ++v)
      if (before(s_c[v], s_d[v], c, d)) c = s_c[v], d = s_d[v];
    if (tid == 0) off[k] = d;
    prev = a + d;
    // the next frame writes s_c / s_d only after its own first barrier, which every thread reaches after reading them here
  }
}

struct AddParams {
  const float* x;
  const int32_t* offsets;
  float* y;
  const float* window;
  const ittm_row* rows;
  int64_t x_elems, offsets_elems, y_elems;
};

__global__ void __launch_bounds__(OWG) overlap_add(AddParams p) {
  const ittm_row row = p.rows[blockIdx.y];
  if (row_refusal(row, p.x_elems, p.offsets_elems, p.y_elems)) return;
  const int64_t S = row.speed, n = row.n;
  const int64_t n_out = out_len(n, S);
  const int64_t m = (int64_t)blockIdx.x * ITTM_RUN + PER * (int64_t)threadIdx.x;   // this thread's outputs are m .. m + 3
  if (m >= n_out) return;
  const int64_t k0 = m / HOP;                                // (k0 + 1 <= (n_out - 1) / HOP + 1 = K - 1)
  const int j = (int)(m - k0 * HOP);
  const int32_t* off = p.offsets + row.o_off;
  const int64_t from_a = nominal(k0, S) + off[k0] + HOP + j;  // the falling half: where frame k0 goes on
  const int64_t from_b = nominal(k0 + 1, S) + off[k0 + 1] + j; // the rising half: frame k0 + 1
  const f32x4 wa = *reinterpret_cast<const f32x4*>(p.window + HOP + j);
  const f32x4 wb = *reinterpret_cast<const f32x4*>(p.window + j);
  const float* x = p.x + row.x_off;
  f32x4 v;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int64_t ia = from_a + q, ib = from_b + q;
    const float xa = ia >= 0 && ia < n ? x[ia] : 0.f;
    const float xb = ib >= 0 && ib < n ? x[ib] : 0.f;
    v[q] = fmaf(wb[q], xb, wa[q] * xa);
  }
  float* y = p.y + row.y_off + m;                            // a multiple of 4 elements from y
  if (m + PER <= n_out) {
    *reinterpret_cast<f32x4*>(y) = v;
  } else {
    for (int q = 0; q < PER; ++q)
      if (m + q < n_out) y[q] = v[q];
  }
}

}  // namespace ittm

#define ITTM_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittm::set_error(__VA_ARGS__);  \
      return ITTM_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

static int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ittm::set_error("%s: %s", who, hipGetErrorString(e));
    return ITTM_ERR_LAUNCH;
  }
  return ITTM_OK;
}

// the message of a refused row; `who` is the entry point
static int refuse_row(const char* who, int r, const ittm_row& g, int why, int64_t x_elems, int64_t offsets_elems, int64_t y_elems) {
  using namespace ittm;
  const int64_t n_out = why >= 5 ? out_len(g.n, g.speed) : 0;
  switch (why) {
    case 1: ITTM_REQUIRE(false, "%s: row %d has n = %lld samples (1 <= n < 2^40)", who, r, (long long)g.n);
    case 2: ITTM_REQUIRE(false, "%s: row %d has the speed S = %d (S = round(1024 speed), %d <= S <= %d)", who, r, g.speed, ITTM_SPEED_MIN, ITTM_SPEED_MAX);
    case 3: ITTM_REQUIRE(false, "%s: row %d lies outside x (x_off = %lld, n = %lld, x_elems = %lld)", who, r, (long long)g.x_off, (long long)g.n,
                         (long long)x_elems);
    case 4: ITTM_REQUIRE(false, "%s: row %d has an offset that is no multiple of 4 (x_off = %lld, o_off = %lld, y_off = %lld)", who, r,
                         (long long)g.x_off, (long long)g.o_off, (long long)g.y_off);
    case 5: ITTM_REQUIRE(false, "%s: row %d has K = %lld frames: offsets too small (o_off = %lld, offsets_elems = %lld)", who, r,
                         (long long)frames_of(n_out), (long long)g.o_off, (long long)offsets_elems);
    default: ITTM_REQUIRE(false, "%s: row %d has n_out = %lld outputs: y too small (y_off = %lld, y_elems = %lld)", who, r, (long long)n_out,
                          (long long)g.y_off, (long long)y_elems);
  }
}

extern "C" int ittm_abi_version(void) { return ITTM_ABI_VERSION; }
extern "C" const char* ittm_last_error(void) { return ittm::g_err; }

extern "C" int ittm_search(const ittm_search_args* a, void* stream) {
  using namespace ittm;
  ITTM_REQUIRE(a != nullptr, "ittm_search: null argument struct");
  ITTM_REQUIRE(a->x && a->offsets && a->rows && a->rows_dev, "ittm_search: null pointer");
  ITTM_REQUIRE(aligned(a->x, 16) && aligned(a->offsets, 4) && aligned(a->rows_dev, 8),
               "ittm_search: x must be 16-byte aligned, rows_dev 8-byte aligned, offsets 4-byte aligned");
  ITTM_REQUIRE(a->n_rows >= 1 && a->n_rows <= 65535, "ittm_search: n_rows must be 1..65535 (got %d)", a->n_rows);
  ITTM_REQUIRE(a->x_elems >= 0 && a->offsets_elems >= 0, "ittm_search: negative element count");
  for (int r = 0; r < a->n_rows; ++r) {
    const int why = row_refusal(a->rows[r], a->x_elems, a->offsets_elems, -1);
    if (why) return refuse_row("ittm_search", r, a->rows[r], why, a->x_elems, a->offsets_elems, -1);
  }
  SearchParams p;
  p.x = a->x, p.offsets = a->offsets, p.rows = a->rows_dev;
  p.x_elems = a->x_elems, p.offsets_elems = a->offsets_elems;
  hipLaunchKernelGGL(search, dim3(a->n_rows), dim3(LAGS), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittm_search");
}

extern "C" int ittm_overlap_add(const ittm_overlap_add_args* a, void* stream) {
  using namespace ittm;
  ITTM_REQUIRE(a != nullptr, "ittm_overlap_add: null argument struct");
  ITTM_REQUIRE(a->x && a->offsets && a->y && a->window && a->rows && a->rows_dev, "ittm_overlap_add: null pointer");
  ITTM_REQUIRE(aligned(a->x, 4) && aligned(a->offsets, 4) && aligned(a->y, 16) && aligned(a->window, 16) && aligned(a->rows_dev, 8),
               "ittm_overlap_add: y and window must be 16-byte aligned, rows_dev 8-byte aligned, x and offsets 4-byte aligned");
  ITTM_REQUIRE(a->n_rows >= 1 && a->n_rows <= 65535, "ittm_overlap_add: n_rows must be 1..65535 (got %d)", a->n_rows);
  ITTM_REQUIRE(a->x_elems >= 0 && a->offsets_elems >= 0 && a->y_elems >= 0, "ittm_overlap_add: negative element count");
  {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(a->x), x1 = x0 + 4 * (uintptr_t)a->x_elems;
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(a->y), y1 = y0 + 4 * (uintptr_t)a->y_elems;
    ITTM_REQUIRE(!(x0 < y1 && y0 < x1), "ittm_overlap_add: y overlaps x (an output would be read as a later output's input)");
  }
  int64_t most = 0;
  for (int r = 0; r < a->n_rows; ++r) {
    const int why = row_refusal(a->rows[r], a->x_elems, a->offsets_elems, a->y_elems);
    if (why) return refuse_row("ittm_overlap_add", r, a->rows[r], why, a->x_elems, a->offsets_elems, a->y_elems);
    const int64_t n_out = out_len(a->rows[r].n, a->rows[r].speed);
    if (n_out > most) most = n_out;
  }
  ITTM_REQUIRE((most + ITTM_RUN - 1) / ITTM_RUN <= 0x7fffffff, "ittm_overlap_add: a row of %lld outputs is more than one launch covers", (long long)most);
  AddParams p;
  p.x = a->x, p.offsets = a->offsets, p.y = a->y, p.window = a->window, p.rows = a->rows_dev;
  p.x_elems = a->x_elems, p.offsets_elems = a->offsets_elems, p.y_elems = a->y_elems;
  dim3 grid((unsigned)((most + ITTM_RUN - 1) / ITTM_RUN), a->n_rows);
  hipLaunchKernelGGL(overlap_add, grid, dim3(OWG), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittm_overlap_add");
}
