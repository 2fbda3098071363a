// libindextts_post.so (include/indextts_post.h): waveform finishing for gfx950 between the vocoder's fp32 samples and the PCM
// encoder -- trim silence, cap pauses, set the level (indextts/utils/post_wave.py).  Two streaming
// kernels; the decisions between them (which frames are silent, which pieces stay, the gain) are host integer / float64 logic
// over ~100 frames per second of audio.
//
// frame_stats: grid (frame groups, rows); one workgroup (4 waves) covers ITTP_FRAMES_PER_WG = 16 consecutive frames of ONE
//   row, a wave four of them.  A frame is 240 samples = 60 lanes x one 16-byte load (the four frames of a wave are 3840
//   contiguous bytes; all four loads are issued before the first is used).  Per lane p = x0 x0, then fma(x_i, x_i, p) for
//   i = 1, 2, 3 and the maximum of the four |x_i|; across the wave a butterfly over lane distances 32 .. 1 (sum and max side by
//   side).  Lane 0 of each wave puts its four (sum, peak) pairs into LDS -- the one LDS step -- and after the barrier the
//   workgroup's first 16 threads store the 16 pairs as 128 contiguous bytes.  No atomics; a frame's bits do not depend on where
//   it sits in the launch.
// splice: grid (runs, rows); one workgroup owns ITTP_RUN = 1024 consecutive outputs of ONE row, a thread four of them.  The
//   row's pieces are walked in order with wave-uniform loads (they tile the outputs, so the walk also checks them); a thread
//   whose four outputs lie inside one piece at a 16-byte aligned source address loads them as one 16-byte vector, otherwise
//   sample by sample; away from a fade the weight is the gain alone.  One 16-byte store per thread; the thread that owns the
//   row's last, partial group stores its 1..3 samples one by one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_post.h"

namespace ittp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int WG = 256;
constexpr int WAVES = WG / 64;
constexpr int FPWAVE = ITTP_FRAMES_PER_WG / WAVES;   // frames per wave
constexpr int LANES = ITTP_FRAME / 4;                // lanes of a wave that hold samples
constexpr int PER = ITTP_RUN / WG;                   // outputs per thread
constexpr int64_t MAX_INDEX = (int64_t)1 << 40;
static_assert(FPWAVE * WAVES == ITTP_FRAMES_PER_WG && LANES <= 64 && LANES * 4 == ITTP_FRAME, "a frame is one 16-byte load per lane of one wave");
static_assert(PER == 4, "a thread assembles four samples per store");
static_assert(sizeof(ittp_row) == 16 && sizeof(ittp_piece) == 32 && sizeof(ittp_out_row) == 48, "table layouts of the header");

__host__ __device__ inline int64_t frames_of(int64_t n) { return (n + ITTP_FRAME - 1) / ITTP_FRAME; }

// Why a row of frame_stats is refused (0: it is taken).  The entry point runs this on the host copy of the table and the kernel
// on the device copy: one statement of the range checks.
__host__ __device__ inline int stat_row_refusal(const ittp_row& r, int64_t row, int64_t x_elems, int64_t stats_elems, int64_t stride) {
  if (r.n < 1 || r.n >= MAX_INDEX) return 1;
  if (r.x_off < 0 || (r.x_off & 3) != 0 || r.x_off >= MAX_INDEX || r.x_off + r.n > x_elems) return 2;
  if (stride < 0 || stride >= MAX_INDEX || frames_of(r.n) > stride || 2 * ((row + 1) * stride) > stats_elems) return 3;
  return 0;
}

struct StatParams {
  const float* x;
  float* stats;
  const ittp_row* rows;
  int64_t x_elems, stats_elems, stride;
};

__global__ void __launch_bounds__(WG) frame_stats(StatParams p) {
  __shared__ f32x2 s_out[ITTP_FRAMES_PER_WG];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const ittp_row row = p.rows[blockIdx.y];
  // what the host checked on its copy of the table, again on the one this launch reads
  if (stat_row_refusal(row, blockIdx.y, p.x_elems, p.stats_elems, p.stride)) return;
  const int64_t nf = frames_of(row.n);
  const int64_t f0 = (int64_t)blockIdx.x * ITTP_FRAMES_PER_WG;
  if (f0 >= nf) return;
  const float* x = p.x + row.x_off;

  f32x4 v[FPWAVE];
#pragma unroll
  for (int k = 0; k < FPWAVE; ++k) {
    const int64_t at = (f0 + wave * FPWAVE + k) * ITTP_FRAME + lane * 4;   // (a frame past the row's last starts at or past n)
    v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (lane < LANES) {
      if (at + 3 < row.n) {
        v[k] = *reinterpret_cast<const f32x4*>(x + at);
      } else {
        for (int i = 0; i < 4; ++i)
          if (at + i < row.n) v[k][i] = x[at + i];
      }
    }
  }
  float ss[FPWAVE], pk[FPWAVE];
#pragma unroll
  for (int k = 0; k < FPWAVE; ++k) {
    float s = v[k][0] * v[k][0];
    s = fmaf(v[k][1], v[k][1], s);
    s = fmaf(v[k][2], v[k][2], s);
    s = fmaf(v[k][3], v[k][3], s);
    ss[k] = s;
    pk[k] = fmaxf(fmaxf(fabsf(v[k][0]), fabsf(v[k][1])), fmaxf(fabsf(v[k][2]), fabsf(v[k][3])));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int k = 0; k < FPWAVE; ++k) {
      ss[k] += __shfl_xor(ss[k], d, 64);
      pk[k] = fmaxf(pk[k], __shfl_xor(pk[k], d, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < FPWAVE; ++k) s_out[wave * FPWAVE + k] = f32x2{ss[k], pk[k]};
  }
  __syncthreads();
  if (tid < ITTP_FRAMES_PER_WG && f0 + tid < nf)
    reinterpret_cast<f32x2*>(p.stats)[(int64_t)blockIdx.y * p.stride + f0 + tid] = s_out[tid];
}

// Why a row of splice is refused, and why a piece of it is (0: taken).  Host and kernel, as above.
__host__ __device__ inline int out_row_refusal(const ittp_out_row& r, int64_t x_elems, int64_t y_elems, int n_pieces) {
  if (r.x_off < 0 || r.n_in < 0 || r.x_off >= MAX_INDEX || r.n_in >= MAX_INDEX || r.x_off + r.n_in > x_elems) return 1;
  if (r.y_off < 0 || (r.y_off & 3) != 0 || r.n_out < 0 || r.y_off >= MAX_INDEX || r.n_out >= MAX_INDEX || r.y_off + r.n_out > y_elems) return 2;
  if (r.piece0 < 0 || r.n_pieces < 0 || (int64_t)r.piece0 + r.n_pieces > n_pieces) return 3;
  if (!(fabsf(r.gain) <= 3.0e38f)) return 4;                 // (false for a NaN too)
  return 0;
}

// `end`: where the row's previous piece ended (0 before the first)
__host__ __device__ inline int piece_refusal(const ittp_piece& c, int64_t end, int64_t n_in, int64_t n_out) {
  if ((c.fade_in != 0 && c.fade_in != ITTP_FADE) || (c.fade_out != 0 && c.fade_out != ITTP_FADE)) return 1;
  if (c.n < (int64_t)c.fade_in + c.fade_out) return 2;
  if (c.src_off < 0 || c.n >= MAX_INDEX || c.src_off >= MAX_INDEX || c.src_off + c.n > n_in) return 3;
  if (c.dst_off < end) return 4;
  if (c.dst_off > end) return 5;
  if (c.dst_off + c.n > n_out) return 6;
  return 0;
}

struct SpliceParams {
  const float* x;
  float* y;
  const float* ramp;
  const ittp_out_row* rows;
  const ittp_piece* pieces;
  int64_t x_elems, y_elems;
  int n_pieces;
};

__global__ void __launch_bounds__(WG) splice(SpliceParams p) {
  const ittp_out_row row = p.rows[blockIdx.y];
  if (out_row_refusal(row, p.x_elems, p.y_elems, p.n_pieces)) return;
  const int64_t r0 = (int64_t)blockIdx.x * ITTP_RUN;
  if (r0 >= row.n_out) return;
  const int64_t r1 = min(r0 + ITTP_RUN, row.n_out);
  const int64_t o = r0 + PER * (int64_t)threadIdx.x;         // this thread's outputs are o .. o + 3
  const float* x = p.x + row.x_off;
  const float gain = row.gain;
  float v[PER] = {0.f, 0.f, 0.f, 0.f};
  int64_t end = 0;
  for (int k = 0; k < row.n_pieces; ++k) {                   // (uniform: every lane walks the same pieces)
    const ittp_piece c = p.pieces[row.piece0 + k];
    if (piece_refusal(c, end, row.n_in, row.n_out)) return;  // the device copy is not what the host checked: nothing is written
    end = c.dst_off + c.n;
    if (end <= r0) continue;
    if (c.dst_off >= r1) break;
    const int64_t i0 = o - c.dst_off;                        // where in the piece this thread's first output lies
    if (i0 + PER <= 0 || i0 >= c.n) continue;
    const float* src = x + c.src_off;
    if (i0 >= 0 && i0 + PER <= c.n && (reinterpret_cast<uintptr_t>(src + i0) & 15) == 0) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(src + i0);
      if (i0 >= c.fade_in && i0 + PER <= c.n - c.fade_out) {
#pragma unroll
        for (int q = 0; q < PER; ++q) v[q] = gain * xv[q];
      } else {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const int64_t i = i0 + q;
          const float w = i < c.fade_in ? p.ramp[i] : c.n - 1 - i < c.fade_out ? p.ramp[c.n - 1 - i] : 1.f;
          v[q] = (gain * w) * xv[q];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int64_t i = i0 + q;
        if (i >= 0 && i < c.n) {
          const float w = i < c.fade_in ? p.ramp[i] : c.n - 1 - i < c.fade_out ? p.ramp[c.n - 1 - i] : 1.f;
          v[q] = (gain * w) * src[i];
        }
      }
    }
  }
  if (o >= r1) return;
  float* y = p.y + row.y_off + o;                            // a multiple of 4 elements from y: y_off, r0 and 4 tid are
  if (o + PER <= r1) {
    *reinterpret_cast<f32x4*>(y) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int q = 0; q < PER; ++q)
      if (o + q < r1) y[q] = v[q];
  }
}

}  // namespace ittp

#define ITTP_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittp::set_error(__VA_ARGS__);  \
      return ITTP_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

static int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ittp::set_error("%s: %s", who, hipGetErrorString(e));
    return ITTP_ERR_LAUNCH;
  }
  return ITTP_OK;
}

extern "C" int ittp_abi_version(void) { return ITTP_ABI_VERSION; }
extern "C" const char* ittp_last_error(void) { return ittp::g_err; }

extern "C" int ittp_frame_stats(const ittp_frame_stats_args* a, void* stream) {
  using namespace ittp;
  ITTP_REQUIRE(a != nullptr, "ittp_frame_stats: null argument struct");
  ITTP_REQUIRE(a->x && a->stats && a->rows && a->rows_dev, "ittp_frame_stats: null pointer");
  ITTP_REQUIRE(aligned(a->x, 16) && aligned(a->stats, 8) && aligned(a->rows_dev, 8),
               "ittp_frame_stats: x must be 16-byte aligned, stats and rows_dev 8-byte aligned");
  ITTP_REQUIRE(a->n_rows >= 1 && a->n_rows <= 65535, "ittp_frame_stats: n_rows must be 1..65535 (got %d)", a->n_rows);
  ITTP_REQUIRE(a->x_elems >= 0 && a->stats_elems >= 0 && a->stat_stride >= 1 && a->stat_stride < MAX_INDEX,
               "ittp_frame_stats: negative element count, or stat_stride below 1");
  for (int r = 0; r < a->n_rows; ++r) {
    const ittp_row& g = a->rows[r];
    switch (stat_row_refusal(g, r, a->x_elems, a->stats_elems, a->stat_stride)) {
      case 0: break;
      case 1: ITTP_REQUIRE(false, "ittp_frame_stats: row %d has n = %lld samples (1 <= n < 2^40)", r, (long long)g.n);
      case 2: ITTP_REQUIRE(false, "ittp_frame_stats: row %d lies outside x, or its x_off = %lld is no multiple of 4", r, (long long)g.x_off);
      default: ITTP_REQUIRE(false, "ittp_frame_stats: row %d has %lld frames: stat_stride = %lld, stats_elems = %lld (2 * n_rows * stat_stride floats)", r,
                            (long long)frames_of(g.n), (long long)a->stat_stride, (long long)a->stats_elems);
    }
  }
  StatParams p;
  p.x = a->x, p.stats = a->stats, p.rows = a->rows_dev;
  p.x_elems = a->x_elems, p.stats_elems = a->stats_elems, p.stride = a->stat_stride;
  int64_t most = 0;
  for (int r = 0; r < a->n_rows; ++r) most = frames_of(a->rows[r].n) > most ? frames_of(a->rows[r].n) : most;
  dim3 grid((unsigned)((most + ITTP_FRAMES_PER_WG - 1) / ITTP_FRAMES_PER_WG), a->n_rows);
  hipLaunchKernelGGL(frame_stats, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittp_frame_stats");
}

extern "C" int ittp_splice(const ittp_splice_args* a, void* stream) {
  using namespace ittp;
  ITTP_REQUIRE(a != nullptr, "ittp_splice: null argument struct");
  ITTP_REQUIRE(a->x && a->y && a->ramp && a->rows && a->rows_dev, "ittp_splice: null pointer");
  ITTP_REQUIRE(a->n_rows >= 1 && a->n_rows <= 65535, "ittp_splice: n_rows must be 1..65535 (got %d)", a->n_rows);
  ITTP_REQUIRE(a->n_pieces >= 0 && (a->n_pieces == 0 || (a->pieces && a->pieces_dev)), "ittp_splice: n_pieces = %d with a null piece table", a->n_pieces);
  ITTP_REQUIRE(aligned(a->x, 4) && aligned(a->y, 16) && aligned(a->ramp, 4) && aligned(a->rows_dev, 8) && aligned(a->pieces_dev, 8),
               "ittp_splice: y must be 16-byte aligned, rows_dev and pieces_dev 8-byte aligned, x and ramp 4-byte aligned");
  ITTP_REQUIRE(a->x_elems >= 0 && a->y_elems >= 0, "ittp_splice: negative element count");
  int64_t most = 0;
  for (int r = 0; r < a->n_rows; ++r) {
    const ittp_out_row& g = a->rows[r];
    switch (out_row_refusal(g, a->x_elems, a->y_elems, a->n_pieces)) {
      case 0: break;
      case 1: ITTP_REQUIRE(false, "ittp_splice: row %d lies outside x (x_off = %lld, n_in = %lld, x_elems = %lld)", r, (long long)g.x_off,
                           (long long)g.n_in, (long long)a->x_elems);
      case 2: ITTP_REQUIRE(false, "ittp_splice: row %d lies outside y (y_off = %lld a multiple of 4, y_off + n_out = %lld <= y_elems = %lld)", r,
                           (long long)g.y_off, (long long)(g.y_off + g.n_out), (long long)a->y_elems);
      case 3: ITTP_REQUIRE(false, "ittp_splice: row %d names the pieces [%d, %d + %d) of a table of %d", r, g.piece0, g.piece0, g.n_pieces, a->n_pieces);
      default: ITTP_REQUIRE(false, "ittp_splice: row %d has a gain that is not finite", r);
    }
    int64_t end = 0;
    for (int k = 0; k < g.n_pieces; ++k) {
      const ittp_piece& c = a->pieces[g.piece0 + k];
      switch (piece_refusal(c, end, g.n_in, g.n_out)) {
        case 0: break;
        case 1: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d: fade_in = %d, fade_out = %d (each 0 or ITTP_FADE = %d)", k, r, c.fade_in,
                             c.fade_out, ITTP_FADE);
        case 2: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d is shorter than its fades: n = %lld < fade_in + fade_out = %d", k, r,
                             (long long)c.n, c.fade_in + c.fade_out);
        case 3: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d lies outside its source row: [%lld, %lld) of %lld samples", k, r,
                             (long long)c.src_off, (long long)(c.src_off + c.n), (long long)g.n_in);
        case 4: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d overlaps the destination of the piece before it: dst_off = %lld < %lld", k, r,
                             (long long)c.dst_off, (long long)end);
        case 5: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d leaves a gap in the destination: dst_off = %lld > %lld", k, r,
                             (long long)c.dst_off, (long long)end);
        default: ITTP_REQUIRE(false, "ittp_splice: piece %d of row %d ends past the row's n_out: %lld > %lld", k, r, (long long)(c.dst_off + c.n),
                              (long long)g.n_out);
      }
      end = c.dst_off + c.n;
    }
    ITTP_REQUIRE(end == g.n_out, "ittp_splice: the pieces of row %d cover %lld outputs of n_out = %lld", r, (long long)end, (long long)g.n_out);
    if (g.n_out > most) most = g.n_out;
  }
  if (most == 0) return ITTP_OK;                             // nothing to produce: no launch
  SpliceParams p;
  p.x = a->x, p.y = a->y, p.ramp = a->ramp, p.rows = a->rows_dev, p.pieces = a->pieces_dev;
  p.x_elems = a->x_elems, p.y_elems = a->y_elems, p.n_pieces = a->n_pieces;
  dim3 grid((unsigned)((most + ITTP_RUN - 1) / ITTP_RUN), a->n_rows);
  hipLaunchKernelGGL(splice, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittp_splice");
}
