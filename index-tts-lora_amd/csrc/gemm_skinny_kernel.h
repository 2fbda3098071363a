// The skinny (decode-step) GEMM kernel and its device helpers: shared by gemm_skinny.hip (16-bit and fp32 weights) and
// gemm_skinny_w8.hip (FP8 E4M3 weights, the W8 instantiation family).  The structure is described at the head of gemm_skinny.hip.
#pragma once
#include "common.h"
#include "ln_math.h"
#include <type_traits>

#ifndef ITTS_FOLD_ORDER
#define ITTS_FOLD_ORDER 0   // build-time A/B of the LayerNorm-folded form: 0 = activations requested first, statistics MFMAs under the weight
                            // stream; 1 = weights first, statistics MFMAs behind the main ones
#endif
#ifndef ITTS_NT_WEIGHTS
#define ITTS_NT_WEIGHTS 0   // build-time A/B: non-temporal policy for the once-read weight blocks (measured neutral)
#endif

namespace itts {

template <typename F>
__device__ __forceinline__ F ldw(const void* p) {
  if constexpr (ITTS_NT_WEIGHTS) return ld16_nt<F>(p);
  else return ld16<F>(p);
}

// The kernel's arguments come in two parts.  SKINNY_LEAD: what the first operand requests need -- the weight image, the activations,
// the cache position word, the shape, the split, the packed-x geometry, the waves per workgroup (blockDim.x is itself a word of the
// argument buffer: reading it would put the scalar load back in front of the first request) -- as plain leading parameters, 14 dwords:
// exactly what gfx950 delivers in SGPRs at wave launch (kernarg preload, csrc/Makefile; a by-value struct is never preloaded).
// SkinnyTail: what only the bias / residual requests and the epilogue read, one trailing struct whose scalar load is issued beside
// the first requests and waited for at its first consumer.  SkinnyParams is both, as the launchers fill it and the kernel body
// reads it.
struct SkinnyTail {
  const float* bias;
  void* y;
  float* yf;
  void* kcache;
  void* vcache;
  int epi;
  int heads, smax;
  int slab_rows;
  const int32_t* kv_tab;   // QKV epilogue into a paged cache: block table [rows][ITTS_KV_TAB], or NULL
  int kv_bs_log2;
  const float* cvec;       // FOLD: c_j = sum_k gamma_k W_kj (bias then holds d_j)
  float ln_eps;
  int32_t* bump;           // one device word this launch increments (it must not read it)
  int y_pa;                // packed-activation layout for y
  int y_mtp, y_row0;       // row tiles and first row of a packed y (the rows may land inside a taller packed operand)
  const float* post_scale; // RELU_AFFINE epilogues: y = relu(v) * post_scale[n] + post_shift[n]
  const float* post_shift;
  const float* w_scale;    // W8: one fp32 scale per output column, applied to the accumulator in front of the epilogue
#if ITTS_STAMPS
  unsigned long long* stamps;
#endif
#if ITTS_DIAG
  int exp;   // diagnostic ablations: bit 0 = every activation fragment is k-step 0's (L1-resident), bit 1 = every weight block is block 0
#endif
};

struct SkinnyParams : SkinnyTail {
  const void* wp;
  const void* x;
  const int32_t* pos;      // QKV epilogue: the cache position word; NULL for every other epilogue
  int M, N, K;
  int ksplit;
  int x_pa;                // packed-activation layout for x
  int mtp, row0;           // row tiles of the WHOLE operand, first row of this launch (a multiple of 16)
  int nw;                  // waves per workgroup (the plan's NW; the launch sites pass it)
};
#define SKINNY_LEAD_PARAMS                                                                                               \
  const void* wp, const void* x, const int32_t* pos, int M, int N, int K, int ksplit, int x_pa, int mtp, int row0, int nw
#define SKINNY_LEAD_NAMES wp, x, pos, M, N, K, ksplit, x_pa, mtp, row0, nw
#define SKINNY_LEAD_ARGS(p, q) (p).wp, (p).x, (p).pos, (p).M, (p).N, (p).K, (p).ksplit, (p).x_pa, (p).mtp, (p).row0, (q).NW

#if ITTS_STAMPS
#define ITTS_STAMP(i) ITTS_STAMP_IF(p.stamps != nullptr, i)
#define ITTS_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define ITTS_STAMP(i) do { } while (0)
#define ITTS_STAMP_DRAIN() do { } while (0)
#endif

// 4 consecutive elements of a row; `nval` of them exist (N need not be a multiple of 4: the 8194-column head)
template <typename T>
__device__ __forceinline__ void store4(T* dst, const f32x4& v, int nval) {
  if (nval >= 4 && ((reinterpret_cast<uintptr_t>(dst) & (sizeof(T) * 4 - 1)) == 0)) {
    if constexpr (sizeof(T) == 4) {
      st16(dst, v);
    } else {
      typedef T t4 __attribute__((ext_vector_type(4)));
      t4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = Elem<T>::from_f(v[e]);
      *reinterpret_cast<t4*>(dst) = o;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nval) dst[e] = Elem<T>::from_f(v[e]);
  }
}

__device__ __forceinline__ f32x4 load4f(const float* src, int nval) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (nval >= 4 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) return ld16<f32x4>(src);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < nval) v[e] = src[e];
  return v;
}

// W8: eight E4M3 codes (two dwords, k ascending from the low byte) -> one 16-bit MFMA fragment, exactly (every finite E4M3 value,
// subnormals included, is a bf16 and an f16 value).  The hardware conversion of gfx950 reads the OCP e4m3fn encoding.
#ifndef ITTS_W8_CVT_VIA_F32
#define ITTS_W8_CVT_VIA_F32 0   // build-time A/B: 1 = v_cvt_pk_f32_fp8 and a float -> T pack instead of the direct fp8 -> T conversion
#endif
template <typename T>
__device__ __forceinline__ typename Elem<T>::frag w8_frag(uint32_t lo, uint32_t hi) {
  typedef T t2 __attribute__((ext_vector_type(2)));
  typename Elem<T>::frag f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t v = h == 0 ? lo : hi;
#if ITTS_W8_CVT_VIA_F32
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, true);
    f[4 * h + 0] = (T)a[0];
    f[4 * h + 1] = (T)a[1];
    f[4 * h + 2] = (T)b[0];
    f[4 * h + 3] = (T)b[1];
#else
    t2 a, b;
    if constexpr (std::is_same<T, f16_t>::value) {
      a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, false);
      b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, true);
    } else {
      a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false);
      b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true);
    }
    f[4 * h + 0] = a[0];
    f[4 * h + 1] = a[1];
    f[4 * h + 2] = b[0];
    f[4 * h + 3] = b[1];
#endif
  }
  return f;
}

template <typename F>
__device__ __forceinline__ F ones_frag() {
  F z;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(F) / sizeof(z[0])); ++i) z[i] = 1;
  return z;
}

// NTB = column tiles per workgroup (grids stay within one round of the 256 CUs: a 257th workgroup costs a full second
// round for this kernel), SPW = k-steps a wave keeps in registers per pass, MT = 16-row tiles per workgroup (grid.z walks
// the row tiles of the launch in groups of MT), FOLD = LayerNorm folded into this GEMM (see the head of the file),
// MAXW = most waves per workgroup (16: the register budget of a 1024-thread workgroup, 128 per lane).
// W8 = FP8 E4M3 weights (include/indextts_hip.h): a weight block is still 1 KiB and one 16-byte load per lane, but it covers
// 64 k -- the lane's fragments of TWO activation k-steps, converted to T in registers in front of the MFMAs.  The K walk (split
// over the waves, SPW per pass) then counts weight blocks, each with XPS = 2 activation fragments per row tile; the accumulator
// is multiplied by the column's scale in front of the epilogue.  T is bf16 or f16.
template <typename T, int MT, int SPW, int NTB, bool FOLD, int MAXW, bool W8 = false>
__global__ __launch_bounds__(MAXW * 64) void gemm_skinny_kernel(SKINNY_LEAD_PARAMS, SkinnyTail tail) {
  const SkinnyParams p{tail, SKINNY_LEAD_NAMES};
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  typedef typename std::conditional<W8, u32x4, frag>::type wfrag;   // a lane's 16 bytes of a weight block, as loaded
  constexpr int E = EL::E, KS = EL::KS;
  constexpr int XPS = W8 ? 2 : 1;                                   // activation k-steps per weight block
  static_assert(!W8 || sizeof(T) == 2, "the FP8-weight forms convert to bf16 / f16");
  extern __shared__ __attribute__((aligned(16))) float red[];  // [NW][NTB][MT][64][4] | FOLD: [NW][MT][16][2]
#if ITTS_STAMPS
  unsigned long long st_[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) st_[i] = 0;
  unsigned long long rt0_ = 0;
  if (p.stamps != nullptr && threadIdx.x == 0) rt0_ = __builtin_amdgcn_s_memrealtime();
#endif
  ITTS_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = p.nw;
  const int nt0 = (int)blockIdx.x * NTB, ks = blockIdx.y;
  const int mt0 = (int)blockIdx.z * MT;       // first row tile of this workgroup inside the launch's rows
  const int NTtot = (p.N + 15) / 16;
  const int g = lane >> 4, r = lane & 15;
  const int KTx = p.K / KS;                       // k-steps of the activations
  const int KT = (KTx + XPS - 1) / XPS;           // weight blocks along K (W8: the image is zero-padded to 64 k)
  const int SB = (KT + p.ksplit - 1) / p.ksplit;  // k-steps (W8: weight blocks) per split slice
  const int b_begin = ks * SB, b_end = min(KT, b_begin + SB);
  const int spw = (b_end - b_begin + NW - 1) / NW;
  const int s_begin = b_begin + wave * spw;
  const int s_end = min(b_end, s_begin + spw);

  const char* bp = (const char*)p.wp + ((int64_t)nt0 * KT * 64 + lane) * 16;  // tile t of this workgroup: + t*KT*1024
  const T* X = (const T*)p.x;

  // Epilogue operands of this wave's output units are requested behind the first pass's operand requests, under the weight
  // stream: their latency overlaps it and the epilogue issues no load of its own.  Their addresses are the first thing that needs
  // the trailing argument struct, so its scalar load -- issued at the head, beside the operand requests, which need preloaded
  // arguments only -- is waited for here and not in front of the weight stream.  pre2 = the residual values the RESID epilogue adds
  // to, or (FOLD) c.  UPRE units per wave cover every launch with >= 8 waves; launches with fewer waves (tiny K) finish in a
  // second loop.
  constexpr int UPRE = (NTB * MT + 7) / 8;
  f32x4 bias_pre[UPRE], pre2[UPRE], scale_pre[W8 ? UPRE : 1];
  int pos_pre = 0;
  auto epi_requests = [&]() {
    // range-checked loads: a null bias, another K slice, columns past N (the 8194-column head), rows past M read zeros -- no
    // branch, so no join at which the compiler would wait for this round trip before the weight requests go out
    const __amdgpu_buffer_rsrc_t rbias = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.bias), 0, p.bias != nullptr ? p.N * 4 : 0, 0x00020000);
    const bool resid = !FOLD && p.epi == ITTS_EPI_RESID_F32;
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
        FOLD ? (void*)const_cast<float*>(p.cvec) : (void*)p.yf, 0, FOLD ? p.N * 4 : (resid ? p.M * p.N * 4 : 0), 0x00020000);
#pragma unroll
    for (int ui = 0; ui < UPRE; ++ui) {
      const int u = wave + ui * NW;
      const int t = u / MT, mt = u - t * MT;
      const int col0 = (nt0 + t) * 16 + g * 4, row = (mt0 + mt) * 16 + r;
      const bool uok = u < NTB * MT && col0 < p.N;
      const unsigned boff = (uok && ks == 0) ? (unsigned)col0 * 4u : 0x80000000u;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        bias_pre[ui][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbias, boff + 4u * e, 0, 0));
      const unsigned o2 = !uok ? 0x80000000u : FOLD ? (unsigned)col0 * 4u : (row < p.M ? (unsigned)(row * p.N + col0) * 4u : 0x80000000u);
      pre2[ui] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r2, o2, 0, 0));
    }
  };
  // W8: the columns' scales, the same way (N % 4 != 0: element by element, columns past N read zeros).  Requested with the bias; the
  // forms with more than 16 output units per workgroup (SCALE_LATE: 6 row tiles x 3 column tiles, whose K walk fills the register
  // file) request them behind the K walk, where the accumulators have gone to LDS, and the reduction's barrier covers the trip.
  constexpr bool SCALE_LATE = UPRE > 2;
  auto scale_requests = [&]() {
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w_scale), 0, p.N * 4, 0x00020000);
#pragma unroll
    for (int ui = 0; ui < (W8 ? UPRE : 1); ++ui) {
      const int u = wave + ui * NW;
      const int col0 = (nt0 + u / MT) * 16 + g * 4;
      const unsigned soff = (u < NTB * MT && col0 < p.N) ? (unsigned)col0 * 4u : 0x80000000u;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        scale_pre[ui][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsc, soff + 4u * e, 0, 0));
    }
  };
  // the cache position word (QKV epilogue): its pointer is preloaded, so this request leaves with the first operand requests.  A
  // readable word either way -- a select, no branch, so no join at which the compiler would wait for it in front of them
  pos_pre = *(p.pos != nullptr ? p.pos : (const int32_t*)p.wp);

  f32x4 acc[NTB][MT];
#pragma unroll
  for (int t = 0; t < NTB; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // FOLD: row statistics of the raw rows on the matrix pipe.  s1: ones x frag -> every lane (g, r) holds sum_k h[r][k] in all
  // four elements; s2: frag x frag -> lane (g, r) element e holds sum_k h[4g+e][k] h[r][k], the diagonal (g == r>>2, e == r&3)
  // is sum_k h[r][k]^2.  Exact products of the T-typed values, fp32 accumulation.
  f32x4 s1[FOLD ? MT : 1], s2[FOLD ? MT : 1];
#pragma unroll
  for (int mt = 0; mt < (FOLD ? MT : 1); ++mt) s1[mt] = s2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag ones = ones_frag<frag>();

  // the j-th activation fragment of weight block / k-step s (W8: k-step 2 s + j, which a K % 64 != 0 leaves without rows for the
  // last block's second half: zeros against the image's zero padding)
  auto x_frag = [&](int s, const int j, const int mt) -> frag {
    const int row = (mt0 + mt) * 16 + r;
#if ITTS_DIAG
    if (p.exp & 1) s = s < s_end ? 0 : s;
#endif
    const int xs = s * XPS + j;
    const bool on = s < s_end && (!W8 || xs < KTx);
    if (p.x_pa) {   // one contiguous 1-KiB block per (k-step, row tile); padding rows exist and are never stored
      // 33-64 rows run 4 row tiles, 65-96 run 6: a tile past the operand's last one is not there to be read.  Its rows are past M and
      // never stored, so the operand's last tile stands in (a uniform clamp: no further predicate on the load)
      const int tile = min((p.row0 >> 4) + mt0 + mt, p.mtp - 1);
      return on ? ld16<frag>(X + (((int64_t)xs * p.mtp + tile) * 64 + lane) * E) : zero_frag<frag>();
    }
    return (on && row < p.M) ? ld16<frag>(X + (int64_t)row * p.K + xs * KS + g * E) : zero_frag<frag>();
  };
  auto w_frag = [&](int s, const int t) -> wfrag {
#if ITTS_DIAG
    if (p.exp & 2) s = s < s_end ? 0 : s;
#endif
    return (s < s_end && nt0 + t < NTtot) ? ldw<wfrag>(bp + ((int64_t)t * KT + s) * 1024) : zero_frag<wfrag>();
  };
  // the XPS MFMA A fragments of a loaded weight block
  auto a_frags = [&](const wfrag& b, frag (&wa)[XPS]) {
    if constexpr (W8) {
      wa[0] = w8_frag<T>(b[0], b[1]);
      wa[1] = w8_frag<T>(b[2], b[3]);
    } else {
      wa[0] = b;
    }
  };

  // One pass over SPW k-steps from `base`.  The FIRST pass always runs (a wave without a K share requests nothing and adds
  // zeros): every wave executes one straight line -- operand requests, one wait, MFMAs -- with no join in front of the
  // requests (round 3: together with the branch-free bias preload and the LDS-only barrier, 5.65 -> 5.29 us per launch
  // over a block's four GEMMs against the round-2 kernel on the same box, tools/probes/ab_r02_gemm.py).
  // paged KV cache (QKV epilogue): the block that holds the append position of each of this wave's output rows.  Requested
  // BEHIND the first pass's operand requests (it needs the position word, and nothing before the epilogue needs it), with the
  // other epilogue operands.
  int blk_pre[UPRE];
#pragma unroll
  for (int ui = 0; ui < UPRE; ++ui) blk_pre[ui] = 0;
  auto late_requests = [&]() {
    epi_requests();
    if constexpr (W8 && !SCALE_LATE) scale_requests();
    const int32_t* tp = p.kv_tab != nullptr ? p.kv_tab : (const int32_t*)p.wp;   // a readable word either way: a select, no branch
#pragma unroll
    for (int ui = 0; ui < UPRE; ++ui) {
      const int u = wave + ui * NW;
      const int mt = u % MT;
      const int row = (mt0 + mt) * 16 + r;
      const int idx = (p.kv_tab != nullptr && row < p.M) ? (p.row0 + row) * ITTS_KV_TAB + ((pos_pre >> p.kv_bs_log2) & (ITTS_KV_TAB - 1)) : 0;
      blk_pre[ui] = tp[idx];
    }
  };
  auto k_pass = [&](const int base, auto first_tag) {
    constexpr bool FIRST_PASS = decltype(first_tag)::value;
    wfrag bf[NTB][SPW];
    if constexpr (MT <= 2) {
      frag af[SPW][XPS][MT];
      if constexpr (FOLD && ITTS_FOLD_ORDER == 0) {
        // activations FIRST (vmcnt retires in issue order): the statistics MFMAs below need only them and run while the
        // weight blocks, the long pole from HBM, are still in flight
#pragma unroll
        for (int i = 0; i < SPW; ++i)
#pragma unroll
          for (int j = 0; j < XPS; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[i][j][mt] = x_frag(base + i, j, mt);
      }
#pragma unroll
      for (int t = 0; t < NTB; ++t)
#pragma unroll
        for (int i = 0; i < SPW; ++i) bf[t][i] = w_frag(base + i, t);
      if constexpr (!FOLD || ITTS_FOLD_ORDER != 0) {
#pragma unroll
        for (int i = 0; i < SPW; ++i)
#pragma unroll
          for (int j = 0; j < XPS; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[i][j][mt] = x_frag(base + i, j, mt);
      }
      if constexpr (FIRST_PASS) late_requests();
      ITTS_STAMP(1);
#if ITTS_STAMPS
      ITTS_STAMP_DRAIN();
      ITTS_STAMP(2);
#endif
      auto stats = [&]() {
#pragma unroll
        for (int i = 0; i < SPW; ++i)
#pragma unroll
          for (int j = 0; j < XPS; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              s1[mt] = EL::mma(ones, af[i][j][mt], s1[mt]);
              s2[mt] = EL::mma(af[i][j][mt], af[i][j][mt], s2[mt]);
            }
      };
      if constexpr (FOLD && ITTS_FOLD_ORDER == 0) stats();
#pragma unroll
      for (int i = 0; i < SPW; ++i) {
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
          frag wa[XPS];
          a_frags(bf[t][i], wa);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < XPS; ++j) acc[t][mt] = EL::mma(wa[j], af[i][j][mt], acc[t][mt]);  // weights = A operand
        }
      }
      if constexpr (FOLD && ITTS_FOLD_ORDER != 0) stats();
    } else {
      // more than 32 rows: the activation fragments (L2-resident, shared by every workgroup) are fetched row tile by row
      // tile behind the weight blocks; the unrolled loop lets the loads of tile mt+1 fly under the MFMAs of tile mt
#pragma unroll
      for (int t = 0; t < NTB; ++t)
#pragma unroll
        for (int i = 0; i < SPW; ++i) bf[t][i] = w_frag(base + i, t);
      if constexpr (FIRST_PASS) late_requests();
      ITTS_STAMP(1);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        frag af[SPW][XPS];
#pragma unroll
        for (int i = 0; i < SPW; ++i)
#pragma unroll
          for (int j = 0; j < XPS; ++j) af[i][j] = x_frag(base + i, j, mt);
        if constexpr (FOLD) {
#pragma unroll
          for (int i = 0; i < SPW; ++i)
#pragma unroll
            for (int j = 0; j < XPS; ++j) {
              s1[mt] = EL::mma(ones, af[i][j], s1[mt]);
              s2[mt] = EL::mma(af[i][j], af[i][j], s2[mt]);
            }
        }
#pragma unroll
        for (int i = 0; i < SPW; ++i)
#pragma unroll
          for (int t = 0; t < NTB; ++t) {
            frag wa[XPS];
            a_frags(bf[t][i], wa);
#pragma unroll
            for (int j = 0; j < XPS; ++j) acc[t][mt] = EL::mma(wa[j], af[i][j], acc[t][mt]);
          }
      }
      ITTS_STAMP(2);
    }
  };
  k_pass(s_begin, std::true_type{});
  for (int base = s_begin + SPW; base < s_end; base += SPW) k_pass(base, std::false_type{});
  ITTS_STAMP(3);

  // ---- cross-wave reduction, fixed order.  Lane (g, r) of a tile holds Y[row = mt*16 + r][col = tile*16 + 4g .. 4g+3].
#pragma unroll
  for (int t = 0; t < NTB; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) st16(red + (((wave * NTB + t) * MT + mt) * 64 + lane) * 4, acc[t][mt]);
  float* stat = red + NW * NTB * MT * 256;   // FOLD: [wave][mt][row 0..15] x {sum, sum of squares}
  if constexpr (FOLD) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int e = r & 3;
      const float d2 = e == 0 ? s2[mt][0] : e == 1 ? s2[mt][1] : e == 2 ? s2[mt][2] : s2[mt][3];
      if (g == (r >> 2)) {
        float* sp = stat + ((wave * MT + mt) * 16 + r) * 2;
        sp[0] = s1[mt][0];
        sp[1] = d2;
      }
    }
  }
  if constexpr (W8 && SCALE_LATE) scale_requests();
  // LDS-only wait + raw barrier (__syncthreads() would also drain vmcnt)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  ITTS_STAMP(4);
  // one output unit (column tile t, row tile mt): sum the waves' partial tiles, add the bias, apply the epilogue
  auto unit = [&](const int u, const f32x4 bs, const f32x4 p2, const int blk, const f32x4 sc) {
    const int t = u / MT, mt = u - t * MT;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < NW; ++w) v += ld16<f32x4>(red + (((w * NTB + t) * MT + mt) * 64 + lane) * 4);
    if constexpr (W8) v *= sc;   // the columns' weight scales, in front of everything the epilogue does
    const int row = (mt0 + mt) * 16 + r, col0 = (nt0 + t) * 16 + g * 4;
    if constexpr (FOLD) {
      float S1 = 0.f, S2 = 0.f;
      for (int w = 0; w < NW; ++w) {
        const float* sp = stat + ((w * MT + mt) * 16 + r) * 2;
        S1 += sp[0];
        S2 += sp[1];
      }
      const float inv = 1.0f / (float)p.K;
      const float mean = S1 * inv;
      const float var = fmaxf(fmaf(-mean, mean, S2 * inv), 0.f);
      const float rstd = rsqrtf(var + p.ln_eps);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(rstd, fmaf(-mean, p2[e], v[e]), bs[e]);   // rstd (h W' - mean c) + d
    } else {
      v += bs;
    }
    if (row >= p.M || col0 >= p.N) return;
    const int nval = min(4, p.N - col0);
    switch (p.epi) {
      case ITTS_EPI_STORE:
        store4<T>((T*)p.y + (p.y_pa ? pa_off<T>(p.y_row0 + row, col0, p.y_mtp) : (int64_t)row * p.N + col0), v, nval);
        break;
      case ITTS_EPI_GELU_STORE: {
        f32x4 gv = {gelu_new(v[0]), gelu_new(v[1]), gelu_new(v[2]), gelu_new(v[3])};
        store4<T>((T*)p.y + (p.y_pa ? pa_off<T>(p.y_row0 + row, col0, p.y_mtp) : (int64_t)row * p.N + col0), gv, nval);
      } break;
      case ITTS_EPI_SILU_STORE: {
        f32x4 sv;
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] = v[e] / (1.f + __expf(-v[e]));
        store4<T>((T*)p.y + (p.y_pa ? pa_off<T>(p.y_row0 + row, col0, p.y_mtp) : (int64_t)row * p.N + col0), sv, nval);
      } break;
      case ITTS_EPI_RELU_AFFINE_STORE:
      case ITTS_EPI_RELU_AFFINE_TANH_STORE: {
        // TDNN block of the speaker encoder: BatchNorm (eval: an affine map per channel) BEHIND the ReLU
        const f32x4 sc = load4f(p.post_scale + col0, nval), sh = load4f(p.post_shift + col0, nval);
        f32x4 rv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          rv[e] = fmaf(fmaxf(v[e], 0.f), sc[e], sh[e]);
          if (p.epi == ITTS_EPI_RELU_AFFINE_TANH_STORE) rv[e] = tanhf(rv[e]);
        }
        store4<T>((T*)p.y + (p.y_pa ? pa_off<T>(p.y_row0 + row, col0, p.y_mtp) : (int64_t)row * p.N + col0), rv, nval);
      } break;
      case ITTS_EPI_RESID_F32: {
        // residual stream update, one owner per element (no split-K): the old values were requested with the bias.  The
        // T-typed copy (p.y, optional) is what the next LayerNorm-folded GEMM multiplies.
        if constexpr (!FOLD) {
          const f32x4 nv = p2 + v;
          store4<float>(p.yf + (int64_t)row * p.N + col0, nv, nval);
          if (p.y != nullptr)
            store4<T>((T*)p.y + (p.y_pa ? pa_off<T>(p.y_row0 + row, col0, p.y_mtp) : (int64_t)row * p.N + col0), nv, nval);
        }
      } break;
      case ITTS_EPI_STORE_F32:
        store4<float>(p.yf + (int64_t)row * p.N + col0, v, nval);
        break;
      case ITTS_EPI_SLAB_F32:
        store4<float>(p.yf + ((int64_t)ks * p.slab_rows + row) * p.N + col0, v, nval);
        break;
      case ITTS_EPI_QKV_CACHE: {
        const int D = p.N / 3;   // a 4-column group never straddles q|k|v or a head (all multiples of 64)
        if (col0 < D) {
          store4<T>((T*)p.y + (int64_t)row * D + col0, v, nval);
        } else {
          int cc = col0 - D;
          T* cache = (T*)(cc < D ? p.kcache : p.vcache);
          if (cc >= D) cc -= D;
          const int hh = cc >> 6, dd = cc & 63;
          const int64_t at = p.kv_tab == nullptr
                                 ? (((int64_t)row * p.heads + hh) * p.smax + pos_pre) * 64
                                 : ((((int64_t)blk * p.heads + hh) << p.kv_bs_log2) + (pos_pre & ((1 << p.kv_bs_log2) - 1))) * 64;
          store4<T>(cache + at + dd, v, nval);
        }
      } break;
    }
  };
#pragma unroll
  for (int ui = 0; ui < UPRE; ++ui) {
    const int u = wave + ui * NW;
    if (u < NTB * MT) unit(u, bias_pre[ui], pre2[ui], blk_pre[ui], scale_pre[W8 ? ui : 0]);
  }
  for (int u = wave + UPRE * NW; u < NTB * MT; u += NW) {   // fewer than 8 waves (tiny K): the remaining units
    f32x4 bs = {0.f, 0.f, 0.f, 0.f}, p2 = bs, sc = bs;
    const int t = u / MT, mt = u - t * MT;
    const int col0 = (nt0 + t) * 16 + g * 4, row = (mt0 + mt) * 16 + r;
    if (col0 < p.N) {
      if constexpr (W8) sc = load4f(p.w_scale + col0, p.N - col0);
      if (p.bias != nullptr && ks == 0) bs = load4f(p.bias + col0, p.N - col0);
      if constexpr (FOLD) p2 = load4f(p.cvec + col0, p.N - col0);
      else if (p.epi == ITTS_EPI_RESID_F32 && row < p.M) p2 = load4f(p.yf + (int64_t)row * p.N + col0, p.N - col0);
    }
    int blk = 0;
    if (p.kv_tab != nullptr && row < p.M)
      blk = p.kv_tab[(p.row0 + row) * ITTS_KV_TAB + ((pos_pre >> p.kv_bs_log2) & (ITTS_KV_TAB - 1))];
    unit(u, bs, p2, blk, sc);
  }
  // the loop-state word this launch advances (nothing in this launch reads it)
  if (p.bump != nullptr && tid == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) p.bump[0] += 1;
  ITTS_STAMP(5);
#if ITTS_STAMPS
  if (p.stamps != nullptr && threadIdx.x == 0) {
    ITTS_STAMP_DRAIN();
    unsigned long long te_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(te_)::"memory");
    unsigned xcc_;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));
    unsigned long long* o_ = p.stamps + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16;
#pragma unroll
    for (int i = 0; i < 10; ++i) o_[i] = st_[i];
    o_[10] = te_;
    o_[11] = rt0_;
    o_[12] = __builtin_amdgcn_s_memrealtime();
    o_[13] = xcc_ & 0xF;
  }
#endif
}

// Launch geometry of one skinny GEMM (shared by the launchers and by tools through itts_skinny_plan / itts_skinny_plan_w8)
struct SkinnyPlan {
  int NW, spw, ntb, gx, gy, gz, SPWc, MT;
  size_t lds;
};

// The row-tile rule (the launchers and the plan entry points): of `m` rows still to do, one launch takes *rows of them and covers
// them with the returned number of 16-row tiles, the MTall of plan_skinny.  fp32: 16 rows, one tile.  16-bit: up to 96 rows as 1 /
// 2 / 4 / 6 tiles in every workgroup; more than 96 rows go 96 at a time or, with rows_per_wg > 0, all in one launch (plan_skinny
// deals the tiles to grid.z).
static int skinny_row_tiles(int dtype, int m, int rows_per_wg, int* rows) {
  const int cap = dtype == ITTS_F32 ? 16 : (rows_per_wg > 0 && m > 96) ? m : 96;
  const int r = *rows = m < cap ? m : cap;
  return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : r <= 96 ? 6 : (r + 15) / 16;
}

#if ITTS_DIAG
extern int g_tune_ntb, g_tune_nw;   // diagnostic build: itts_debug_set(1|2, v) overrides of the 16-bit / fp32 plan (0 = heuristic)
#endif

// The K walk of a form: KT steps of the walk's unit (a k-step of KS columns; FP8: a 64-k weight block), and the two register-chunk
// classes -- steps a wave keeps per pass.  The FP8 classes 3 / 5 blocks are 6 / 10 activation fragments per row tile: the register
// classes of the 16-bit kernel's 5- and 10-step forms with half the weight registers, so one set of column-tile limits serves both.
struct SkinnyWalk {
  int KT, c_lo, c_hi;
  bool can_fold;   // fp32 has no folded form: the launcher refuses it
  bool w8;         // no split-K, no 16-wave form
};
template <typename T>
static SkinnyWalk skinny_walk(int K) {
  return {K / Elem<T>::KS, 5, 10, sizeof(T) == 2, false};
}
static SkinnyWalk skinny_walk_w8(int K) {
  return {(K / 32 + 1) / 2, 3, 5, true, true};
}

// MTall = 16-row tiles of the launch; rows_per_wg (0 = all of them in every workgroup, else 16 / 32: the row tiles are dealt
// to grid.z -- more, lighter workgroups for the GEMMs that run WITHOUT split-K); wide: up to 16 waves per workgroup (a hint:
// ignored by the folded and the FP8 forms, which have no 16-wave instantiation)
static SkinnyPlan plan_skinny(const SkinnyWalk& w, int N, int ksplit, int MTall, int rows_per_wg, bool wide, bool fold) {
  fold = fold && w.can_fold;
  wide = wide && !fold && !w.w8;   // a folded launch never takes 16 waves
  SkinnyPlan q;
  int MT = MTall;
  if (rows_per_wg > 0 && rows_per_wg / 16 < MTall) MT = rows_per_wg / 16;
  const int gz = (MTall + MT - 1) / MT;
  const int SB = (w.KT + ksplit - 1) / ksplit;
  // waves per workgroup: 8 whenever the slice has 8 k-steps (measured: the split-K 3 out-projection, 14 k-steps, takes
  // 3.8 us with 8 waves x 2 steps against 4.4 us with 3 waves x 5; more than 8 waves change nothing there).  `wide`: 16 waves
  // when that keeps the slice to ONE pass of <= 10 k-steps per wave (a second pass is a second memory round trip)
  int NW = SB > 8 ? 8 : SB;
  if (wide && MT == 1 && SB > 80) NW = 16;
  if (NW < 1) NW = 1;
#if ITTS_DIAG
  if (g_tune_nw > 0 && !w.w8) NW = g_tune_nw > 8 ? 8 : g_tune_nw;
#endif
  const int spw = (SB + NW - 1) / NW;
  const int NT = (N + 15) / 16;
  int ntb = (NT * ksplit * gz + 255) / 256;   // keep the grid within one round of the 256 CUs
#if ITTS_DIAG
  if (g_tune_ntb > 0 && !w.w8) ntb = g_tune_ntb;
#endif
  const int SPWc = spw <= w.c_lo ? w.c_lo : w.c_hi;   // register-chunk variant
  const bool big = SPWc == w.c_hi;
  const int ntb_max = (fold && MT <= 2 && !big) ? 4 : 3;   // 4 tiles: the folded GEMMs of a many-row step with the rows dealt to grid.z
  if (ntb > ntb_max) ntb = ntb_max;
  if (big && ntb > 2) ntb = 2;            // register budget of the big-chunk variant
  if (MT > 2 && big) ntb = 1;             // 4-6 row tiles with big chunks: accumulators + weight fragments
  if (NW == 16) ntb = 1;                  // 128 registers per lane
  if (fold && MT > 2 && ntb > 2) ntb = 2; // the statistics accumulators take 8 registers per row tile
  q.NW = NW;
  q.spw = spw;
  q.ntb = ntb;
  q.SPWc = SPWc;
  q.MT = MT;
  q.gx = (NT + ntb - 1) / ntb;
  q.gy = ksplit;
  q.gz = gz;
  q.lds = (size_t)NW * ntb * MT * 256 * 4 + (fold ? (size_t)NW * MT * 32 * 4 : 0);
  if (q.lds < 1024) q.lds = 1024;
  return q;
}

// the out8 words of itts_skinny_plan / itts_skinny_plan_w8
static int skinny_plan_out8(const SkinnyPlan& q, int* out8) {
  out8[0] = q.gx; out8[1] = q.gy; out8[2] = q.NW; out8[3] = q.ntb; out8[4] = q.spw; out8[5] = (int)q.lds; out8[6] = q.gz; out8[7] = q.MT;
  return ITTS_OK;
}

// The argument check of itts_gemm_skinny and itts_gemm_skinny_w8 (`who` in every message).  w8: the entry point is built for FP8
// weights -- it needs w_scale, bf16 / f16 activations, no split-K and one of the decode step's epilogues; the 16-bit entry point
// refuses w_scale instead.  Out: the split-K factor, the row tiles of a packed y and log2 of the paged cache's block size.
static int skinny_check(const itts_skinny_args* a, const char* who, bool w8, int* ksplit_out, int* y_mtp_out, int* kv_bs_log2_out) {
  ITTS_REQUIRE(a && a->wp && a->x, "%s: null args", who);
  if (w8) {
    ITTS_REQUIRE(a->w_scale, "%s: w_scale is null", who);
    ITTS_REQUIRE(a->dtype == ITTS_BF16 || a->dtype == ITTS_F16, "%s: the activation type must be bf16 or f16 (dtype %d)", who, a->dtype);
    ITTS_REQUIRE(a->ksplit <= 1, "%s: ksplit=%d is not built (the FP8 forms run without split-K)", who, a->ksplit);
  } else {
    ITTS_REQUIRE(!a->w_scale, "%s: w_scale is set: FP8 weights go to itts_gemm_skinny_w8", who);
  }
  const int ks = a->dtype == ITTS_F32 ? 16 : 32;
  ITTS_REQUIRE(a->M >= 0 && a->N > 0 && a->K > 0 && a->K % ks == 0, "%s: bad shape M=%d N=%d K=%d (K %% %d != 0)", who, a->M, a->N, a->K, ks);
  const int ksplit = a->ksplit > 0 ? a->ksplit : 1;
  ITTS_REQUIRE(ksplit <= a->K / ks && ksplit <= 64, "%s: ksplit=%d too large", who, ksplit);
  ITTS_REQUIRE(ksplit == 1 || a->epi == ITTS_EPI_SLAB_F32, "%s: ksplit > 1 requires the slab epilogue", who);
  // (the block size is checked where the table is used: the QKV epilogue)
  const int kv_bs_log2 = kv_block_log2(a->epi == ITTS_EPI_QKV_CACHE && a->kv_tab != nullptr, a->kv_bs);
  const bool slab = a->epi == ITTS_EPI_SLAB_F32 && !w8;
  const bool store = a->epi == ITTS_EPI_STORE || a->epi == ITTS_EPI_GELU_STORE;
  const bool affine = (a->epi == ITTS_EPI_RELU_AFFINE_STORE || a->epi == ITTS_EPI_RELU_AFFINE_TANH_STORE) && !w8;
  const bool store_any = store || ((a->epi == ITTS_EPI_SILU_STORE || affine) && !w8);
  if (a->epi == ITTS_EPI_QKV_CACHE)
    ITTS_REQUIRE(a->y && a->kcache && a->vcache && a->pos && a->N % 3 == 0 && a->N / 3 == a->heads * 64 &&
                     (a->kv_tab != nullptr ? kv_bs_log2 >= 0 : a->smax > 0),
                 "%s: bad QKV epilogue arguments (paged cache: kv_bs must be 16, 32 or 64)", who);
  else if (a->epi == ITTS_EPI_RESID_F32 || a->epi == ITTS_EPI_STORE_F32 || slab)
    ITTS_REQUIRE(a->yf, "%s: yf is null", who);
  else if (w8)
    ITTS_REQUIRE(store && a->y, "%s: epilogue %d is not built (STORE, GELU_STORE, RESID_F32, QKV_CACHE, STORE_F32)", who, a->epi);
  else
    ITTS_REQUIRE(store_any && a->y, "%s: bad epilogue %d", who, a->epi);
  if (affine) ITTS_REQUIRE(a->post_scale && a->post_shift, "%s: the ReLU + affine epilogues need post_scale and post_shift", who);
  if (a->epi == ITTS_EPI_RESID_F32)
    ITTS_REQUIRE(a->N % 4 == 0 && (int64_t)a->M * a->N < (1ll << 29), "%s: the residual epilogue needs N %% 4 == 0", who);
  if (a->ln_c != nullptr) {
    const bool ok = a->bias && a->N % 4 == 0 && a->epi != ITTS_EPI_RESID_F32;
    if (w8)
      ITTS_REQUIRE(ok, "%s: the LayerNorm-folded form needs bias (= d), N %% 4 == 0, a storing epilogue", who);
    else
      ITTS_REQUIRE(ok && ksplit == 1 && a->epi != ITTS_EPI_SLAB_F32 && a->dtype != ITTS_F32,
                   "%s: the LayerNorm-folded form needs ksplit 1, bias (= d), N %% 4 == 0, a storing epilogue, bf16 / f16", who);
  }
  ITTS_REQUIRE(a->rows_per_wg == 0 || a->rows_per_wg == 16 || a->rows_per_wg == 32, "%s: rows_per_wg must be 0, 16 or 32", who);
  if (a->y_packed) {
    const bool ok = (store_any || a->epi == ITTS_EPI_RESID_F32) && a->N % ks == 0 && a->y;
    if (w8)
      ITTS_REQUIRE(ok, "%s: a packed y needs the STORE / GELU_STORE / RESID_F32 epilogue and N %% 32 == 0", who);
    else
      ITTS_REQUIRE(ok, "%s: a packed y needs the STORE / GELU_STORE / SILU_STORE / RESID_F32 epilogue and N %% %d == 0", who, ks);
  }
  const int y_mtp = a->y_mtp > 0 ? a->y_mtp : (a->M + 15) / 16;
  ITTS_REQUIRE(a->y_row0 >= 0 && a->y_row0 % 16 == 0 && (!a->y_packed || a->y_row0 + a->M <= y_mtp * 16) &&
                   (a->y_packed || (a->y_row0 == 0 && a->y_mtp == 0)),
               "%s: y_row0 / y_mtp place the rows of a PACKED y inside a taller operand (y_row0 %% 16 == 0)", who);
  ITTS_REQUIRE(a->x_mtp == 0 || (a->x_packed && a->x_mtp * 16 >= a->M), "%s: x_mtp is for a packed x of at least M rows", who);
  ITTS_REQUIRE(a->M <= 96 || a->rows_per_wg == 0 || (a->M + 15) / 16 / (a->rows_per_wg / 16) < 65535, "%s: too many rows", who);
  *ksplit_out = ksplit;
  *y_mtp_out = y_mtp;
  *kv_bs_log2_out = kv_bs_log2;
  return ITTS_OK;
}

// The SkinnyParams of one launch over rows [r0, r0 + rows) of the call `a`: operand and output pointers advanced to the chunk, the
// packed-layout geometry, the KV append, the folded LayerNorm and the vectors only some forms read (the affine epilogues', the FP8
// weight scales: NULL where the entry point refuses or ignores them).  esz = bytes of a T element.  Split-K and the diagnostic
// build's words are set by the 16-bit entry point.
static SkinnyParams skinny_params_of(const itts_skinny_args* a, int r0, int rows, size_t esz, int y_mtp, int kv_bs_log2) {
  SkinnyParams p;
  p.M = rows;
  p.N = a->N;
  p.K = a->K;
  p.wp = a->wp;
  p.bias = a->bias;
  p.x = a->x_packed ? (const char*)a->x : (const char*)a->x + (size_t)r0 * a->K * esz;
  p.x_pa = a->x_packed ? 1 : 0;
  p.y_pa = a->y_packed ? 1 : 0;
  p.mtp = a->x_mtp > 0 ? a->x_mtp : (a->M + 15) / 16;
  p.row0 = r0;
  p.y_mtp = y_mtp;
  p.y_row0 = r0 + a->y_row0;
  p.epi = a->epi;
  const size_t ycols = a->epi == ITTS_EPI_QKV_CACHE ? (size_t)a->N / 3 : (size_t)a->N;
  p.y = a->y ? (a->y_packed ? (char*)a->y : (char*)a->y + (size_t)r0 * ycols * esz) : nullptr;
  p.yf = a->yf ? a->yf + (size_t)r0 * a->N : nullptr;
  const size_t crow = (size_t)a->heads * a->smax * 64 * esz;
  const bool paged = a->kv_tab != nullptr;   // (the table row, not the cache pointer, carries the chunk's first row)
  p.kcache = a->kcache ? (char*)a->kcache + (paged ? 0 : (size_t)r0 * crow) : nullptr;
  p.vcache = a->vcache ? (char*)a->vcache + (paged ? 0 : (size_t)r0 * crow) : nullptr;
  p.kv_tab = a->kv_tab;
  p.kv_bs_log2 = kv_bs_log2;
  p.pos = a->epi == ITTS_EPI_QKV_CACHE ? a->pos : nullptr;
  p.nw = 0;   // (the launch sites pass the plan's NW)
  p.heads = a->heads;
  p.smax = a->smax;
  p.ksplit = 1;
  p.slab_rows = a->M;
  p.cvec = a->ln_c;
  p.ln_eps = a->ln_eps > 0.f ? a->ln_eps : 1e-5f;
  p.bump = r0 == 0 ? a->bump : nullptr;
  p.post_scale = a->post_scale;
  p.post_shift = a->post_shift;
  p.w_scale = a->w_scale;
#if ITTS_STAMPS
  p.stamps = nullptr;
#endif
#if ITTS_DIAG
  p.exp = 0;
#endif
  return p;
}

}  // namespace itts
