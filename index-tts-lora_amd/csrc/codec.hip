// libindextts_codec.so (include/indextts_codec.h): the acoustic tokenizer for gfx950 -- the DVAE encoder's convolutions and the
// nearest-code search, fp32 (indextts/vqvae/dvae.py).  Three kernels; the header states the algorithm.
//
// Both launches are one tiled GEMM on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32: per accumulator a k-ordered fma chain):
//   a workgroup of 4 waves owns a 64 x 64 tile of (rows) x (output channels | codes), a wave a 32 x 32 quarter of it as 2 x 2
//   accumulators of 16 x 16 (four independent chains: the pipe's issue rate).  K goes by in steps of 32: the A tile [64][32] and
//   the B tile [32][64] are fetched with 16-byte global loads into registers while the previous step computes, and staged in LDS
//   -- A rows at a pitch of 34 words and B rows at a pitch of 80, so that the 32 lanes of a half-wave that read one operand
//   column (A[l & 15][l >> 4], B[l >> 4][l & 15]) hit 32 different banks.  Two barriers a step.
// conv: grid (row tiles of the longest clip, column tiles, clips).  The A tile is gathered: element (t, k = tap Cin + c) is row
//   t stride + tap - pad of the clip, channel c, or zero outside the clip and in the K padding (Cin is a multiple of 4, so a
//   16-byte group never straddles a tap).  A tile lies inside one clip, so no clip sees another's rows.  Epilogue from the
//   accumulators: bias, residual, ReLU, 64-byte runs of stores.
// nearest: grid (row tiles, code ranges).  A workgroup streams its ITTC_CODE_RANGE codes 64 at a time, each over the whole of D,
//   and keeps per lane the running (score, code) of the 8 rows its accumulators hold; at the end a butterfly over the 16 lanes
//   of a row, then LDS over the two waves that share the rows.  One range: the codes are written.  More: the ranges' winners go
//   to ws and `merge` (a thread per row) walks them in rising order.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_codec.h"

namespace ittc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int BM = 64, BN = 64, BK = ITTC_KSTEP, WG = 256;
constexpr int LDA = BK + 2;                          // pitch of an A row in LDS (words): 2 r + k over a half-wave is 32 banks
constexpr int LDB = BN + 16;                         // pitch of a B row: 16 k + c likewise
constexpr int64_t MAX_ROWS = (int64_t)1 << 40;
constexpr int MAX_CH = 65536;
static_assert(BK == 32 && BM * BK == 2 * WG * 4 && BK * BN == 2 * WG * 4, "a thread stages two 16-byte groups of each tile");
static_assert(ITTC_CODE_RANGE % BN == 0, "a code range is whole tiles");
static_assert(sizeof(ittc_seg) == 32, "table layout of the header");

__host__ __device__ inline int64_t out_rows(int64_t x_len, int stride) { return (x_len + stride - 1) / stride; }
__host__ __device__ inline int64_t packed_k(int taps, int Cin) { return ((int64_t)taps * Cin + BK - 1) / BK * BK; }

// Why a clip is refused (0: it is taken).  The entry point runs this on the host copy of the table and the kernel on the device
// copy: one statement of the range checks.
__host__ __device__ inline int seg_refusal(const ittc_seg& s, int64_t x_rows, int64_t y_rows, int stride) {
  if (s.x_len < 1 || s.x_len >= ((int64_t)1 << 31)) return 1;
  if (s.x_row0 < 0 || s.x_row0 > x_rows - s.x_len) return 2;
  if (s.y_row0 < 0 || s.y_row0 > y_rows - out_rows(s.x_len, stride)) return 3;
  return 0;
}

// is the code j1 of score s1 chosen before j2 of s2?  the larger score; of equal scores the smaller code
__device__ inline bool before(float s1, int j1, float s2, int j2) { return s1 > s2 || (s1 == s2 && j1 < j2); }

// acc += A B over `ksteps` steps of BK, for this wave's 32 x 32 quarter of the workgroup's tile.  la(r, k): the four elements
// k .. k + 3 of tile row r of A (k absolute, a multiple of 4); lb(k, c): the elements c .. c + 3 of row k of B (c in the tile).
template <class LA, class LB>
__device__ inline void tile_gemm(f32x4 (&acc)[2][2], int ksteps, LA la, LB lb, float* As, float* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int ar = tid >> 3, ak = (tid & 7) * 4;       // this thread's groups of the A tile: rows ar and ar + 32, k ak .. ak + 3
  const int bk = tid >> 4, bc = (tid & 15) * 4;      // ... of the B tile: rows bk and bk + 16, columns bc .. bc + 3
  f32x4 ra[2], rb[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) ra[q] = la(ar + 32 * q, ak), rb[q] = lb(bk + 16 * q, bc);
  const float* a_rd = As + (wm * 32 + (lane & 15)) * LDA + (lane >> 4);
  const float* b_rd = Bs + (lane >> 4) * LDB + wn * 32 + (lane & 15);
  for (int ks = 0; ks < ksteps; ++ks) {
    __syncthreads();                                 // every wave is done reading the previous step's tiles
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float* d = As + (ar + 32 * q) * LDA + ak;      // (8-byte aligned: LDA and ak are even)
      *reinterpret_cast<f32x2*>(d) = f32x2{ra[q][0], ra[q][1]};
      *reinterpret_cast<f32x2*>(d + 2) = f32x2{ra[q][2], ra[q][3]};
      *reinterpret_cast<f32x4*>(Bs + (bk + 16 * q) * LDB + bc) = rb[q];
    }
    __syncthreads();
    if (ks + 1 < ksteps) {
      const int k0 = (ks + 1) * BK;
#pragma unroll
      for (int q = 0; q < 2; ++q) ra[q] = la(ar + 32 * q, k0 + ak), rb[q] = lb(k0 + bk + 16 * q, bc);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const float a0 = a_rd[kk], a1 = a_rd[16 * LDA + kk];
      const float b0 = b_rd[kk * LDB], b1 = b_rd[kk * LDB + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

struct ConvParams {
  const float* x;
  const float* w;
  const float* bias;
  const float* resid;
  float* y;
  const ittc_seg* segs;
  int64_t x_rows, y_rows;
  int Cin, Cout, taps, stride, flags, ksteps;
};

__global__ void __launch_bounds__(WG) conv(ConvParams p) {
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  const ittc_seg seg = p.segs[blockIdx.z];
  // what the host checked on its copy of the table, again on the one this launch reads
  if (seg_refusal(seg, p.x_rows, p.y_rows, p.stride)) return;
  const int64_t y_len = out_rows(seg.x_len, p.stride);
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  if (m0 >= y_len) return;                           // (the grid covers the longest clip)
  const int n0 = blockIdx.y * BN;
  const int K = p.taps * p.Cin, pad = (p.taps - 1) / 2;
  const bool relu_in = (p.flags & ITTC_RELU_IN) != 0;
  const float* x = p.x + seg.x_row0 * p.Cin;
  auto la = [&](int r, int k) -> f32x4 {
    const int64_t t = m0 + r;
    if (t >= y_len || k >= K) return f32x4{0.f, 0.f, 0.f, 0.f};
    const int tap = k / p.Cin, c = k - tap * p.Cin;
    const int64_t i = t * p.stride + tap - pad;
    if (i < 0 || i >= seg.x_len) return f32x4{0.f, 0.f, 0.f, 0.f};   // outside the clip: zero, never the neighbour's row
    f32x4 v = *reinterpret_cast<const f32x4*>(x + i * p.Cin + c);
    if (relu_in) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
    return v;
  };
  auto lb = [&](int k, int c) -> f32x4 {
    if (n0 + c >= p.Cout) return f32x4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const f32x4*>(p.w + (int64_t)k * p.Cout + n0 + c);
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  tile_gemm(acc, p.ksteps, la, lb, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  float* y = p.y + seg.y_row0 * p.Cout;
  const float* resid = (p.flags & ITTC_RESIDUAL) ? p.resid + seg.y_row0 * p.Cout : nullptr;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + wn * 32 + ni * 16 + (lane & 15);
    if (col >= p.Cout) continue;
    const float b = p.bias[col];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t t = m0 + wm * 32 + mi * 16 + (lane >> 4) * 4 + e;
        if (t >= y_len) continue;
        float v = acc[mi][ni][e] + b;
        if (resid) v += resid[t * p.Cout + col];
        if (p.flags & ITTC_RELU_OUT) v = fmaxf(v, 0.f);
        y[t * p.Cout + col] = v;
      }
  }
}

struct NearParams {
  const float* z;
  const float* embed;
  const float* h;
  int32_t* code;
  float* score;
  float* ws_s;
  int32_t* ws_j;
  int64_t n_rows;
  int D, J, n_split, ksteps;
};

__global__ void __launch_bounds__(WG) nearest(NearParams p) {
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  __shared__ float red_s[2][BM];
  __shared__ int red_j[2][BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int split = blockIdx.y;
  const int j_lo = split * ITTC_CODE_RANGE;
  const int j_hi = p.J - j_lo < ITTC_CODE_RANGE ? p.J : j_lo + ITTC_CODE_RANGE;
  float best_s[2][4];
  int best_j[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) best_s[mi][e] = -__builtin_huge_valf(), best_j[mi][e] = 0x7fffffff;
  auto la = [&](int r, int k) -> f32x4 {
    if (m0 + r >= p.n_rows || k >= p.D) return f32x4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const f32x4*>(p.z + (m0 + r) * p.D + k);
  };
  for (int n0 = j_lo; n0 < j_hi; n0 += BN) {
    auto lb = [&](int k, int c) -> f32x4 {
      if (k >= p.D || n0 + c >= j_hi) return f32x4{0.f, 0.f, 0.f, 0.f};
      return *reinterpret_cast<const f32x4*>(p.embed + (int64_t)k * p.J + n0 + c);
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_gemm(acc, p.ksteps, la, lb, As, Bs);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int j = n0 + wn * 32 + ni * 16 + (lane & 15);
      if (j >= j_hi) continue;                       // the last, partial tile of a codebook that is no multiple of 64
      const float hj = p.h[j];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = acc[mi][ni][e] - hj;
          if (before(s, j, best_s[mi][e], best_j[mi][e])) best_s[mi][e] = s, best_j[mi][e] = j;
        }
    }
  }
  // a row's 16 lanes (the same lane >> 4), then the two waves that hold the same rows
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = best_s[mi][e];
      int j = best_j[mi][e];
#pragma unroll
      for (int m = 1; m <= 8; m <<= 1) {
        const float os = __shfl_xor(s, m, 64);
        const int oj = __shfl_xor(j, m, 64);
        if (before(os, oj, s, j)) s = os, j = oj;
      }
      if ((lane & 15) == 0) {
        const int r = wm * 32 + mi * 16 + (lane >> 4) * 4 + e;
        red_s[wn][r] = s, red_j[wn][r] = j;
      }
    }
  __syncthreads();
  if (tid < BM && m0 + tid < p.n_rows) {
    float s = red_s[0][tid];
    int j = red_j[0][tid];
    if (before(red_s[1][tid], red_j[1][tid], s, j)) s = red_s[1][tid], j = red_j[1][tid];
    const int64_t row = m0 + tid;
    if (p.n_split == 1) {
      p.code[row] = j < p.J ? j : 0;                 // (no score compared: not finite.  Still a code of the book)
      if (p.score) p.score[row] = s;
    } else {
      p.ws_s[(int64_t)split * p.n_rows + row] = s;
      p.ws_j[(int64_t)split * p.n_rows + row] = j;
    }
  }
}

__global__ void __launch_bounds__(WG) merge(NearParams p) {
  const int64_t row = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (row >= p.n_rows) return;
  float s = p.ws_s[row];
  int j = p.ws_j[row];
  for (int q = 1; q < p.n_split; ++q) {              // range by range, in rising order
    const float os = p.ws_s[(int64_t)q * p.n_rows + row];
    const int oj = p.ws_j[(int64_t)q * p.n_rows + row];
    if (before(os, oj, s, j)) s = os, j = oj;
  }
  p.code[row] = j >= 0 && j < p.J ? j : 0;
  if (p.score) p.score[row] = s;
}

}  // namespace ittc

#define ITTC_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittc::set_error(__VA_ARGS__);  \
      return ITTC_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

static bool overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + 4 * (uintptr_t)a_elems;
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + 4 * (uintptr_t)b_elems;
  return a0 < b1 && b0 < a1;
}

static int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ittc::set_error("%s: %s", who, hipGetErrorString(e));
    return ITTC_ERR_LAUNCH;
  }
  return ITTC_OK;
}

extern "C" int ittc_abi_version(void) { return ITTC_ABI_VERSION; }
extern "C" const char* ittc_last_error(void) { return ittc::g_err; }

extern "C" int ittc_conv(const ittc_conv_args* a, void* stream) {
  using namespace ittc;
  ITTC_REQUIRE(a != nullptr, "ittc_conv: null argument struct");
  const bool res = (a->flags & ITTC_RESIDUAL) != 0;
  ITTC_REQUIRE(a->x && a->w && a->bias && a->y && a->segs && a->segs_dev && (a->resid || !res), "ittc_conv: null pointer");
  ITTC_REQUIRE(aligned(a->x, 16) && aligned(a->w, 16) && aligned(a->bias, 16) && aligned(a->y, 16) && (!res || aligned(a->resid, 16)) &&
                   aligned(a->segs_dev, 8),
               "ittc_conv: x, w, bias, resid and y must be 16-byte aligned, segs_dev 8-byte aligned");
  ITTC_REQUIRE((a->flags & ~(ITTC_RELU_IN | ITTC_RELU_OUT | ITTC_RESIDUAL)) == 0, "ittc_conv: unknown flags 0x%x", a->flags);
  ITTC_REQUIRE(a->taps == 1 || a->taps == 3, "ittc_conv: taps = %d (1 or 3)", a->taps);
  ITTC_REQUIRE(a->stride == 1 || a->stride == 2, "ittc_conv: stride = %d (1 or 2)", a->stride);
  ITTC_REQUIRE(a->Cin >= 4 && a->Cin <= MAX_CH && a->Cin % 4 == 0 && a->Cout >= 4 && a->Cout <= MAX_CH && a->Cout % 4 == 0,
               "ittc_conv: Cin = %d, Cout = %d (multiples of 4 in 4 .. %d)", a->Cin, a->Cout, MAX_CH);
  const int64_t Kpad = packed_k(a->taps, a->Cin);
  ITTC_REQUIRE(a->w_elems == Kpad * a->Cout,
               "ittc_conv: the pack does not match: w_elems = %lld, but taps = %d, Cin = %d, Cout = %d pack to [%lld][%d] = %lld elements",
               (long long)a->w_elems, a->taps, a->Cin, a->Cout, (long long)Kpad, a->Cout, (long long)(Kpad * a->Cout));
  ITTC_REQUIRE(a->n_seg >= 1 && a->n_seg <= 65535, "ittc_conv: n_seg must be 1..65535 (got %d)", a->n_seg);
  ITTC_REQUIRE(a->x_rows >= 0 && a->x_rows < MAX_ROWS && a->y_rows >= 0 && a->y_rows < MAX_ROWS, "ittc_conv: row counts must be in [0, 2^40)");
  ITTC_REQUIRE(!overlap(a->y, a->y_rows * a->Cout, a->x, a->x_rows * a->Cin), "ittc_conv: y overlaps x (an output would be read as another output's input)");
  ITTC_REQUIRE(!res || !overlap(a->y, a->y_rows * a->Cout, a->resid, a->y_rows * a->Cout), "ittc_conv: y overlaps resid");
  int64_t most = 0;
  for (int s = 0; s < a->n_seg; ++s) {
    const ittc_seg& g = a->segs[s];
    switch (seg_refusal(g, a->x_rows, a->y_rows, a->stride)) {
      case 0: break;
      case 1: ITTC_REQUIRE(false, "ittc_conv: segment %d has x_len = %lld rows (1 <= x_len < 2^31)", s, (long long)g.x_len);
      case 2: ITTC_REQUIRE(false, "ittc_conv: segment %d lies outside x (x_row0 = %lld, x_len = %lld, x_rows = %lld)", s, (long long)g.x_row0,
                           (long long)g.x_len, (long long)a->x_rows);
      default: ITTC_REQUIRE(false, "ittc_conv: segment %d lies outside y (y_row0 = %lld, y_len = %lld, y_rows = %lld)", s, (long long)g.y_row0,
                            (long long)out_rows(g.x_len, a->stride), (long long)a->y_rows);
    }
    const int64_t y_len = out_rows(g.x_len, a->stride);
    if (y_len > most) most = y_len;
  }
  ConvParams p;
  p.x = a->x, p.w = a->w, p.bias = a->bias, p.resid = res ? a->resid : nullptr, p.y = a->y, p.segs = a->segs_dev;
  p.x_rows = a->x_rows, p.y_rows = a->y_rows;
  p.Cin = a->Cin, p.Cout = a->Cout, p.taps = a->taps, p.stride = a->stride, p.flags = a->flags, p.ksteps = (int)(Kpad / BK);
  dim3 grid((unsigned)((most + BM - 1) / BM), (unsigned)((a->Cout + BN - 1) / BN), (unsigned)a->n_seg);
  hipLaunchKernelGGL(conv, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittc_conv");
}

extern "C" int ittc_nearest_code(const ittc_nearest_code_args* a, void* stream) {
  using namespace ittc;
  ITTC_REQUIRE(a != nullptr, "ittc_nearest_code: null argument struct");
  ITTC_REQUIRE(a->z && a->embed && a->h && a->code, "ittc_nearest_code: null pointer");
  ITTC_REQUIRE(aligned(a->z, 16) && aligned(a->embed, 16) && aligned(a->h, 16) && aligned(a->code, 4) && aligned(a->score, 4),
               "ittc_nearest_code: z, embed and h must be 16-byte aligned, code and score 4-byte aligned");
  ITTC_REQUIRE(a->n_rows >= 1 && a->n_rows < ((int64_t)1 << 31) - 64, "ittc_nearest_code: n_rows must be in [1, 2^31 - 64) (got %lld)",
               (long long)a->n_rows);
  ITTC_REQUIRE(a->D >= 4 && a->D <= MAX_CH && a->D % 4 == 0, "ittc_nearest_code: D = %d (a multiple of 4 in 4 .. %d)", a->D, MAX_CH);
  ITTC_REQUIRE(a->J >= 4 && a->J <= (1 << 24) && a->J % 4 == 0, "ittc_nearest_code: J = %d (a multiple of 4 in 4 .. 2^24)", a->J);
  const int n_split = (a->J + ITTC_CODE_RANGE - 1) / ITTC_CODE_RANGE;
  if (n_split > 1) {
    const int64_t need = 8 * a->n_rows * n_split;
    ITTC_REQUIRE(a->ws != nullptr && aligned(a->ws, 16), "ittc_nearest_code: J = %d codes are %d ranges: ws must be a 16-byte aligned buffer", a->J, n_split);
    ITTC_REQUIRE(a->ws_bytes >= need, "ittc_nearest_code: ws too small (%lld bytes, %lld rows in %d ranges need %lld)", (long long)a->ws_bytes,
                 (long long)a->n_rows, n_split, (long long)need);
  }
  NearParams p;
  p.z = a->z, p.embed = a->embed, p.h = a->h, p.code = a->code, p.score = a->score;
  p.ws_s = static_cast<float*>(a->ws);
  p.ws_j = n_split > 1 ? reinterpret_cast<int32_t*>(p.ws_s + a->n_rows * n_split) : nullptr;
  p.n_rows = a->n_rows, p.D = a->D, p.J = a->J, p.n_split = n_split, p.ksteps = (a->D + BK - 1) / BK;
  dim3 grid((unsigned)((a->n_rows + BM - 1) / BM), (unsigned)n_split);
  hipLaunchKernelGGL(nearest, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  int rc = launched("ittc_nearest_code");
  if (rc != ITTC_OK || n_split == 1) return rc;
  hipLaunchKernelGGL(merge, dim3((unsigned)((a->n_rows + WG - 1) / WG)), dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  return launched("ittc_nearest_code");
}
