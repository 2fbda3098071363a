// libindextts_score.so (include/indextts_score.h): likelihood scoring for gfx950 -- nll, rank, lse and best of given codes under an
// output head, the [rows][vocabulary] logits never stored (indextts/gpt/score.py).  Three kernels; the
// header states the quantities and the order of every sum.
//
// head: grid (row tiles, column ranges), as codec.hip's `nearest`.  A workgroup of 4 waves owns a 64 x 64 tile of (rows) x
//   (columns), a wave a 32 x 32 quarter of it as 2 x 2 accumulators of 16 x 16, and streams its ITTL_RANGE columns 64 at a time,
//   each over the whole of D.  From the accumulators every lane folds its 8 rows x 2 columns into running values held in
//   registers: (m, s) of the log-sum-exp, the count of columns beating t[r], the best (logit, id).  At the end a butterfly over
//   the 16 lanes of a row, then LDS over the two waves that share the rows.  One range: the outputs are written.  More: the
//   partial results go to ws and `merge` (a thread per row) walks them in rising order.
//   fp32 form: the tile loop of codec.hip on v_mfma_f32_16x16x4_f32: K by 32, A [64][32] at a pitch of 34 words and B [32][64] at a
//     pitch of 80, so that the 32 lanes of a half-wave reading one operand column hit 32 banks.
//   16-bit form: v_mfma_f32_16x16x32_{bf16,f16}: K by 64 (two matrix steps).  x is rounded to the weight type on its way into LDS.
//     Both tiles lie in LDS as [64 rows | columns][64 k] 16-bit, a row = 8 chunks of 16 bytes = one operand fragment each; W is
//     k-major in memory, so a thread that fetched 8 columns of rows k, k + 1 writes 8 dwords (one k pair of one column each):
//     the transpose happens in the write.  Chunk q of row r lies at chunk q ^ ((r ^ (r >> 3)) & 7): the 32 lanes of a half-wave's
//     write (8 column groups x 4 k pairs) then hit 32 banks, and the 16 lanes of a fragment read 16 different 16-byte slots.
// target: a wave per 16 rows; the gathered columns W[:, y[r]] are the B operand of the same matrix instructions, the diagonal the result.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_score.h"

namespace ittl {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int BM = 64, BN = 64, WG = 256;
constexpr int BK = 32;                               // fp32 form: K step
constexpr int LDA = BK + 2;                          // pitch of an A row in LDS (words): 2 r + k over a half-wave is 32 banks
constexpr int LDB = BN + 16;                         // pitch of a B row: 16 k + c likewise
constexpr int BK16 = 64;                             // 16-bit form: K step (two matrix steps of 32)
constexpr int SMEM_F32 = (BM * LDA + BK * LDB) * 4, SMEM_16 = (BM + BN) * BK16 * 2;
constexpr int SMEM = SMEM_F32 > SMEM_16 ? SMEM_F32 : SMEM_16;
constexpr int MAX_D = 65536, MAX_V = 1 << 24;
static_assert(BK == 32 && BM * BK == 2 * WG * 4 && BK * BN == 2 * WG * 4, "fp32: a thread stages two 16-byte groups of each tile");
static_assert(BM * BK16 == WG * 16 && BK16 * BN == WG * 16, "16-bit: a thread stages 16 elements of each tile");
static_assert(ITTL_RANGE % BN == 0, "a column range is whole tiles");
static_assert(ITTL_WS_PER_ROW_RANGE == 20, "five 4-byte values per row and range");

template <class T>
struct Half;
template <>
struct Half<__bf16> {
  typedef bf16x8 frag;
  typedef bf16x2 pair;
  static __device__ inline f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct Half<_Float16> {
  typedef f16x8 frag;
  typedef f16x2 pair;
  static __device__ inline f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// is the column j1 of logit s1 chosen before j2 of s2?  the larger logit; of equal logits the smaller column
__device__ inline bool before(float s1, int j1, float s2, int j2) { return s1 > s2 || (s1 == s2 && j1 < j2); }

// the exponential of the header: 2^(v log2 e)
__device__ inline float E(float v) { return __expf(v); }

// (m, s) <- (m, s) joined with the one logit v
__device__ inline void join_logit(float& m, float& s, float v) {
  if (v > m) {
    s = __fadd_rn(__fmul_rn(s, E(m - v)), 1.f);
    m = v;
  } else if (v != -__builtin_huge_valf()) {           // (a logit of -inf adds nothing, also while m is still -inf; NaN goes on)
    s = __fadd_rn(s, E(v - m));
  }
}

// (m, s) <- (m, s) joined with (m2, s2)
__device__ inline void join(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  const float e1 = m == mm ? 1.f : E(m - mm), e2 = m2 == mm ? 1.f : E(m2 - mm);
  s = __fadd_rn(__fmul_rn(s, e1), __fmul_rn(s2, e2));
  m = mm;
}

// element offset of chunk q (8 elements) of row r in a 16-bit LDS tile [64][64]
__device__ inline int sw(int r, int q) { return r * BK16 + ((q ^ ((r ^ (r >> 3)) & 7)) << 3); }

// fp32: acc += A B over `ksteps` steps of BK, for this wave's 32 x 32 quarter of the workgroup's tile.  la(r, k): the four elements
// k .. k + 3 of tile row r of A (k absolute, a multiple of 4); lb(k, c): the elements c .. c + 3 of row k of B (c in the tile).
template <class LA, class LB>
__device__ inline void tile_gemm_f32(f32x4 (&acc)[2][2], int ksteps, LA la, LB lb, float* As, float* Bs) {
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

// 16-bit: the same over steps of BK16.  la as above (fp32, rounded here); lb(k, c): the 8 elements c .. c + 7 of row k of B.
template <class T, class LA, class LB>
__device__ inline void tile_gemm_16(f32x4 (&acc)[2][2], int ksteps, LA la, LB lb, T* As, T* Bs) {
  typedef typename Half<T>::frag frag;
  typedef typename Half<T>::pair pair;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int ar = tid >> 2, aq = (tid & 3) * 2;       // this thread's part of the A tile: row ar, chunks aq and aq + 1 (16 k)
  const int kp = tid >> 3, cg = tid & 7;             // ... of the B tile: rows 2 kp and 2 kp + 1, columns 8 cg .. 8 cg + 7
  f32x4 ra[4];
  frag rb[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) ra[q] = la(ar, aq * 8 + 4 * q);
#pragma unroll
  for (int q = 0; q < 2; ++q) rb[q] = lb(2 * kp + q, 8 * cg);
  for (int ks = 0; ks < ksteps; ++ks) {
    __syncthreads();                                 // every wave is done reading the previous step's tiles
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      frag f;
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = (T)ra[2 * h][i], f[4 + i] = (T)ra[2 * h + 1][i];
      *reinterpret_cast<frag*>(As + sw(ar, aq + h)) = f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)                      // column 8 cg + i, elements k = 2 kp and 2 kp + 1 of it: one dword
      *reinterpret_cast<pair*>(Bs + sw(8 * cg + i, kp >> 2) + (kp & 3) * 2) = pair{rb[0][i], rb[1][i]};
    __syncthreads();
    if (ks + 1 < ksteps) {
      const int k0 = (ks + 1) * BK16;
#pragma unroll
      for (int q = 0; q < 4; ++q) ra[q] = la(ar, k0 + aq * 8 + 4 * q);
#pragma unroll
      for (int q = 0; q < 2; ++q) rb[q] = lb(k0 + 2 * kp + q, 8 * cg);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = 4 * s + (lane >> 4);             // lane l holds k = 32 s + 8 (l >> 4) .. + 7 of row | column l & 15
      const frag a0 = *reinterpret_cast<const frag*>(As + sw(wm * 32 + (lane & 15), q));
      const frag a1 = *reinterpret_cast<const frag*>(As + sw(wm * 32 + 16 + (lane & 15), q));
      const frag b0 = *reinterpret_cast<const frag*>(Bs + sw(wn * 32 + (lane & 15), q));
      const frag b1 = *reinterpret_cast<const frag*>(Bs + sw(wn * 32 + 16 + (lane & 15), q));
      acc[0][0] = Half<T>::mma(a0, b0, acc[0][0]);
      acc[0][1] = Half<T>::mma(a0, b1, acc[0][1]);
      acc[1][0] = Half<T>::mma(a1, b0, acc[1][0]);
      acc[1][1] = Half<T>::mma(a1, b1, acc[1][1]);
    }
  }
}

struct HeadParams {
  const float* x;
  const void* w;
  const float* b;
  const int32_t* y;
  const float* t;
  float* nll;
  float* lse;
  int32_t* best;
  int32_t* rank;
  float* ws_m;                                       // [n_split][n_rows] each
  float* ws_s;
  float* ws_bs;
  int32_t* ws_cnt;
  int32_t* ws_bj;
  int64_t n_rows;
  int D, V, ldw, n_split;
};

// the outputs of one row from its joined running values
__device__ inline void finish(const HeadParams& p, int64_t row, float m, float s, int cnt, int bj) {
  const int y = p.y[row];
  const bool real = y >= 0 && y < p.V;
  const float lse = m + logf(s);
  p.lse[row] = lse;
  p.best[row] = bj >= 0 && bj < p.V ? bj : 0;        // (no logit compared: none was a number.  Still a column of the head)
  p.nll[row] = real ? lse - p.t[row] : 0.f;
  p.rank[row] = real ? cnt : -1;
}

template <class T>
__global__ void __launch_bounds__(WG) head(HeadParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
  __shared__ float red_m[2][BM], red_s[2][BM], red_bs[2][BM];
  __shared__ int red_cnt[2][BM], red_bj[2][BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int split = blockIdx.y;
  const int j_lo = split * ITTL_RANGE;
  const int j_hi = p.V - j_lo < ITTL_RANGE ? p.V : j_lo + ITTL_RANGE;
  float run_m[2][4], run_s[2][4], best_s[2][4], tgt[2][4];
  int best_j[2][4], cnt[2][4], yy[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      run_m[mi][e] = -__builtin_huge_valf(), run_s[mi][e] = 0.f, cnt[mi][e] = 0;
      best_s[mi][e] = -__builtin_huge_valf(), best_j[mi][e] = 0x7fffffff;
      const int64_t row = m0 + wm * 32 + mi * 16 + (lane >> 4) * 4 + e;
      int y = row < p.n_rows ? p.y[row] : -1;
      if (y < 0 || y >= p.V) y = -1;                 // ignored: no column is counted against it
      yy[mi][e] = y;
      tgt[mi][e] = y >= 0 ? p.t[row] : 0.f;
    }
  auto la = [&](int r, int k) -> f32x4 {
    if (m0 + r >= p.n_rows || k >= p.D) return f32x4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const f32x4*>(p.x + (m0 + r) * p.D + k);
  };
  for (int n0 = j_lo; n0 < j_hi; n0 += BN) {
    f32x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 4) {
      const float* w = static_cast<const float*>(p.w);
      auto lb = [&](int k, int c) -> f32x4 {         // (a group inside the pitch is read whole: columns >= V never leave acc)
        if (k >= p.D || n0 + c >= p.ldw) return f32x4{0.f, 0.f, 0.f, 0.f};
        return *reinterpret_cast<const f32x4*>(w + (int64_t)k * p.ldw + n0 + c);
      };
      float* As = reinterpret_cast<float*>(smem);
      tile_gemm_f32(acc, (p.D + BK - 1) / BK, la, lb, As, As + BM * LDA);
    } else {
      typedef typename Half<T>::frag frag;
      const T* w = static_cast<const T*>(p.w);
      auto lb = [&](int k, int c) -> frag {
        frag z;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = (T)0.f;
        if (k >= p.D || n0 + c >= p.ldw) return z;
        return *reinterpret_cast<const frag*>(w + (int64_t)k * p.ldw + n0 + c);
      };
      T* As = reinterpret_cast<T*>(smem);
      tile_gemm_16<T>(acc, (p.D + BK16 - 1) / BK16, la, lb, As, As + BM * BK16);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int j = n0 + wn * 32 + ni * 16 + (lane & 15);
      if (j >= j_hi) continue;                       // past V (the pad columns of the pitch among them): never into a result
      const float bj = p.b[j];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float l = acc[mi][ni][e] + bj;
          join_logit(run_m[mi][e], run_s[mi][e], l);
          if (before(l, j, best_s[mi][e], best_j[mi][e])) best_s[mi][e] = l, best_j[mi][e] = j;
          const int y = yy[mi][e];
          if (y >= 0 && j != y && before(l, j, tgt[mi][e], y)) ++cnt[mi][e];
        }
    }
  }
  // a row's 16 lanes (the same lane >> 4), then the two waves that hold the same rows
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float m = run_m[mi][e], s = run_s[mi][e], bs = best_s[mi][e];
      int bj = best_j[mi][e], c = cnt[mi][e];
#pragma unroll
      for (int d = 1; d <= 8; d <<= 1) {
        const float om = __shfl_xor(m, d, 64), os = __shfl_xor(s, d, 64), obs = __shfl_xor(bs, d, 64);
        const int obj = __shfl_xor(bj, d, 64), oc = __shfl_xor(c, d, 64);
        join(m, s, om, os);
        if (before(obs, obj, bs, bj)) bs = obs, bj = obj;
        c += oc;
      }
      if ((lane & 15) == 0) {
        const int r = wm * 32 + mi * 16 + (lane >> 4) * 4 + e;
        red_m[wn][r] = m, red_s[wn][r] = s, red_bs[wn][r] = bs, red_bj[wn][r] = bj, red_cnt[wn][r] = c;
      }
    }
  __syncthreads();
  if (tid < BM && m0 + tid < p.n_rows) {
    float m = red_m[0][tid], s = red_s[0][tid], bs = red_bs[0][tid];
    int bj = red_bj[0][tid], c = red_cnt[0][tid] + red_cnt[1][tid];
    join(m, s, red_m[1][tid], red_s[1][tid]);
    if (before(red_bs[1][tid], red_bj[1][tid], bs, bj)) bs = red_bs[1][tid], bj = red_bj[1][tid];
    const int64_t row = m0 + tid;
    if (p.n_split == 1) {
      finish(p, row, m, s, c, bj);
    } else {
      const int64_t at = (int64_t)split * p.n_rows + row;
      p.ws_m[at] = m, p.ws_s[at] = s, p.ws_bs[at] = bs, p.ws_bj[at] = bj, p.ws_cnt[at] = c;
    }
  }
}

__global__ void __launch_bounds__(WG) merge(HeadParams p) {
  const int64_t row = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (row >= p.n_rows) return;
  float m = p.ws_m[row], s = p.ws_s[row], bs = p.ws_bs[row];
  int bj = p.ws_bj[row], c = p.ws_cnt[row];
  for (int q = 1; q < p.n_split; ++q) {              // range by range, in rising order
    const int64_t at = (int64_t)q * p.n_rows + row;
    join(m, s, p.ws_m[at], p.ws_s[at]);
    const float obs = p.ws_bs[at];
    const int obj = p.ws_bj[at];
    if (before(obs, obj, bs, bj)) bs = obs, bj = obj;
    c += p.ws_cnt[at];
  }
  finish(p, row, m, s, c, bj);
}

struct TargetParams {
  const float* x;
  const void* w;
  const float* b;
  const int32_t* y;
  float* t;
  int64_t n_rows;
  int D, V, ldw;
};

// One wave per 16 rows, on the matrix pipe: B column c of the 16 x 16 product is column y[row c] of W, so the diagonal holds the
// rows' target logits -- by the instructions, the operand layout and the k order of `head`, hence with its bits.
template <class T>
__global__ void __launch_bounds__(WG) target(TargetParams p) {
  const int lane = threadIdx.x & 63, g = lane >> 4;
  const int64_t row = ((int64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * 16 + (lane & 15);
  const bool live = row < p.n_rows;
  int y = live ? p.y[row] : -1;
  const bool real = y >= 0 && y < p.V;
  if (!real) y = 0;                                  // the only use of a target as an index is behind this check
  const float* x = p.x + (live ? row : 0) * p.D;
  const T* w = static_cast<const T*>(p.w) + y;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (sizeof(T) == 4) {
    for (int k0 = 0; k0 < p.D; k0 += 4) {            // lane l: A[row l & 15][k0 + (l >> 4)], B[k0 + (l >> 4)][column l & 15]
      const int k = k0 + g;
      const float a = live ? x[k] : 0.f;
      const float b = (float)w[(int64_t)k * p.ldw];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
  } else {
    typedef typename Half<T>::frag frag;
    for (int k0 = 0; k0 < p.D; k0 += 32) {           // lane l: k = k0 + 8 (l >> 4) .. + 7 of row | column l & 15
      const int k = k0 + 8 * g;
      frag a, b;
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = (T)0.f, b[i] = (T)0.f;
      if (k < p.D) {                                 // (D is a multiple of 8: a fragment is inside or outside)
        if (live) {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(x + k), hi = *reinterpret_cast<const f32x4*>(x + k + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) a[i] = (T)lo[i], a[4 + i] = (T)hi[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = w[(int64_t)(k + i) * p.ldw];
      }
      acc = Half<T>::mma(a, b, acc);
    }
  }
  // the product's element (row r, column c) is register r & 3 of lane 16 (r >> 2) + c: the diagonal
  if (live && g == (lane & 15) >> 2) {
    const int e = lane & 3;
    const float d = e == 0 ? acc[0] : e == 1 ? acc[1] : e == 2 ? acc[2] : acc[3];
    p.t[row] = real ? d + p.b[y] : 0.f;
  }
}

}  // namespace ittl

#define ITTL_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ittl::set_error(__VA_ARGS__);  \
      return ITTL_ERR_INVALID;       \
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
    ittl::set_error("%s: %s", who, hipGetErrorString(e));
    return ITTL_ERR_LAUNCH;
  }
  return ITTL_OK;
}

// the checks both entry points share (0: taken)
static int check_common(const char* who, const float* x, const void* w, const float* b, const int32_t* y, int64_t n_rows, int D, int V, int ldw,
                        int dtype) {
  using namespace ittl;
  ITTL_REQUIRE(x && w && b && y, "%s: null pointer (x, w, b, y)", who);
  ITTL_REQUIRE(aligned(x, 16) && aligned(w, 16) && aligned(b, 4) && aligned(y, 4), "%s: x and w must be 16-byte aligned, b and y 4-byte aligned", who);
  ITTL_REQUIRE(dtype == ITTL_F32 || dtype == ITTL_BF16 || dtype == ITTL_F16, "%s: dtype = %d (ITTL_F32, ITTL_BF16 or ITTL_F16)", who, dtype);
  const int dm = dtype == ITTL_F32 ? 4 : 8;
  ITTL_REQUIRE(D >= dm && D <= MAX_D && D % dm == 0, "%s: D = %d (a multiple of %d in %d .. %d)", who, D, dm, dm, MAX_D);
  ITTL_REQUIRE(V >= 1 && V <= MAX_V, "%s: V = %d (1 .. 2^24)", who, V);
  ITTL_REQUIRE(ldw >= V && ldw % 8 == 0 && ldw <= MAX_V + 8, "%s: ldw = %d (the pitch of W: a multiple of 8, >= V = %d)", who, ldw, V);
  ITTL_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31) - 64, "%s: n_rows must be in [1, 2^31 - 64) (got %lld)", who, (long long)n_rows);
  return ITTL_OK;
}

// does the output `o` of o_bytes overlap one of the inputs?  (the name of the input, or NULL)
static const char* overlaps_input(const void* o, int64_t o_bytes, const float* x, const void* w, const float* b, const int32_t* y, const float* t,
                                  int64_t n_rows, int D, int V, int ldw, int dtype) {
  const int64_t esz = dtype == ITTL_F32 ? 4 : 2;
  if (overlap(o, o_bytes, x, 4 * n_rows * D)) return "x";
  if (overlap(o, o_bytes, w, esz * (int64_t)D * ldw)) return "w";
  if (overlap(o, o_bytes, b, 4 * (int64_t)V)) return "b";
  if (overlap(o, o_bytes, y, 4 * n_rows)) return "y";
  if (t && overlap(o, o_bytes, t, 4 * n_rows)) return "t";
  return nullptr;
}

extern "C" int ittl_abi_version(void) { return ITTL_ABI_VERSION; }
extern "C" const char* ittl_last_error(void) { return ittl::g_err; }

extern "C" int ittl_target_logit(const ittl_target_logit_args* a, void* stream) {
  using namespace ittl;
  ITTL_REQUIRE(a != nullptr, "ittl_target_logit: null argument struct");
  if (int rc = check_common("ittl_target_logit", a->x, a->w, a->b, a->y, a->n_rows, a->D, a->V, a->ldw, a->dtype)) return rc;
  ITTL_REQUIRE(a->t != nullptr && aligned(a->t, 4), "ittl_target_logit: t must be a 4-byte aligned buffer");
  const char* in = overlaps_input(a->t, 4 * a->n_rows, a->x, a->w, a->b, a->y, nullptr, a->n_rows, a->D, a->V, a->ldw, a->dtype);
  ITTL_REQUIRE(in == nullptr, "ittl_target_logit: t overlaps %s", in);
  TargetParams p;
  p.x = a->x, p.w = a->w, p.b = a->b, p.y = a->y, p.t = a->t, p.n_rows = a->n_rows, p.D = a->D, p.V = a->V, p.ldw = a->ldw;
  const dim3 grid((unsigned)((a->n_rows + WG / 4 - 1) / (WG / 4)));   // 4 waves of 16 rows
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->dtype == ITTL_F32) hipLaunchKernelGGL(target<float>, grid, dim3(WG), 0, st, p);
  else if (a->dtype == ITTL_BF16) hipLaunchKernelGGL(target<__bf16>, grid, dim3(WG), 0, st, p);
  else hipLaunchKernelGGL(target<_Float16>, grid, dim3(WG), 0, st, p);
  return launched("ittl_target_logit");
}

extern "C" int ittl_head_nll(const ittl_head_nll_args* a, void* stream) {
  using namespace ittl;
  ITTL_REQUIRE(a != nullptr, "ittl_head_nll: null argument struct");
  if (int rc = check_common("ittl_head_nll", a->x, a->w, a->b, a->y, a->n_rows, a->D, a->V, a->ldw, a->dtype)) return rc;
  ITTL_REQUIRE(a->t && a->nll && a->lse && a->best && a->rank, "ittl_head_nll: null pointer (t, nll, lse, best, rank)");
  ITTL_REQUIRE(aligned(a->t, 4) && aligned(a->nll, 4) && aligned(a->lse, 4) && aligned(a->best, 4) && aligned(a->rank, 4),
               "ittl_head_nll: t, nll, lse, best and rank must be 4-byte aligned");
  const int n_split = (a->V + ITTL_RANGE - 1) / ITTL_RANGE;
  const int64_t need = (int64_t)ITTL_WS_PER_ROW_RANGE * a->n_rows * n_split;
  if (n_split > 1) {
    ITTL_REQUIRE(a->ws != nullptr && aligned(a->ws, 16), "ittl_head_nll: V = %d columns are %d ranges: ws must be a 16-byte aligned buffer", a->V, n_split);
    ITTL_REQUIRE(a->ws_bytes >= need, "ittl_head_nll: ws too small (%lld bytes, %lld rows in %d ranges need %lld)", (long long)a->ws_bytes,
                 (long long)a->n_rows, n_split, (long long)need);
  }
  const void* outs[4] = {a->nll, a->lse, a->best, a->rank};
  const char* names[4] = {"nll", "lse", "best", "rank"};
  for (int i = 0; i < 4; ++i) {
    const char* in = overlaps_input(outs[i], 4 * a->n_rows, a->x, a->w, a->b, a->y, a->t, a->n_rows, a->D, a->V, a->ldw, a->dtype);
    ITTL_REQUIRE(in == nullptr, "ittl_head_nll: %s overlaps %s", names[i], in);
    ITTL_REQUIRE(n_split == 1 || !overlap(outs[i], 4 * a->n_rows, a->ws, need), "ittl_head_nll: %s overlaps ws", names[i]);
  }
  if (n_split > 1) {
    const char* in = overlaps_input(a->ws, need, a->x, a->w, a->b, a->y, a->t, a->n_rows, a->D, a->V, a->ldw, a->dtype);
    ITTL_REQUIRE(in == nullptr, "ittl_head_nll: ws overlaps %s", in);
  }
  HeadParams p;
  p.x = a->x, p.w = a->w, p.b = a->b, p.y = a->y, p.t = a->t, p.nll = a->nll, p.lse = a->lse, p.best = a->best, p.rank = a->rank;
  const int64_t n = a->n_rows * n_split;
  p.ws_m = static_cast<float*>(a->ws);
  p.ws_s = n_split > 1 ? p.ws_m + n : nullptr;
  p.ws_bs = n_split > 1 ? p.ws_m + 2 * n : nullptr;
  p.ws_cnt = n_split > 1 ? reinterpret_cast<int32_t*>(p.ws_m + 3 * n) : nullptr;
  p.ws_bj = n_split > 1 ? reinterpret_cast<int32_t*>(p.ws_m + 4 * n) : nullptr;
  p.n_rows = a->n_rows, p.D = a->D, p.V = a->V, p.ldw = a->ldw, p.n_split = n_split;
  const dim3 grid((unsigned)((a->n_rows + BM - 1) / BM), (unsigned)n_split);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->dtype == ITTL_F32) hipLaunchKernelGGL(head<float>, grid, dim3(WG), 0, st, p);
  else if (a->dtype == ITTL_BF16) hipLaunchKernelGGL(head<__bf16>, grid, dim3(WG), 0, st, p);
  else hipLaunchKernelGGL(head<_Float16>, grid, dim3(WG), 0, st, p);
  int rc = launched("ittl_head_nll");
  if (rc != ITTL_OK || n_split == 1) return rc;
  hipLaunchKernelGGL(merge, dim3((unsigned)((a->n_rows + WG - 1) / WG)), dim3(WG), 0, st, p);
  return launched("ittl_head_nll");
}
