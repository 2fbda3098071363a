// libindextts_out.so (include/indextts_out.h): the PCM output back-end for gfx950 -- the vocoder's fp32 samples at 24 kHz -> any
// sample rate -> float / PCM16 / G.711, one launch for any number of rows (indextts/utils/pcm_out.py).
//
// pcm_out: one workgroup (4 waves) per run of up to 1024 consecutive outputs of ONE row.
//   1. the contiguous input span the run needs -- (q_last - q_first) * orig + taps samples from q_first * orig - width -- is
//      staged once in LDS, zeros for the positions outside the utterance ([0, N_total)) on the way: the tap loop has no bounds.
//   2. thread i owns the outputs i, i + 256, i + 512, i + 768 of the run, so that the 64 lanes of a wave are 64 consecutive
//      outputs: they read the tap table, which the host packs TRANSPOSED ([taps][new]), at consecutive addresses (one phase
//      per lane) and the staged samples at a stride of orig / new (a broadcast within a q when new > 1; a stride of orig dwords
//      when new == 1: conflict-free for odd orig).  Four independent fmaf chains per thread, each in ascending t.
//   3. the four results go to LDS; thread i reads the run's outputs 4 i .. 4 i + 3 back as one ds_read_b128, encodes them and
//      stores them with ONE vector store: 16 bytes (f32), 8 (pcm16) or 4 (G.711) per lane, 1 KiB / 512 B / 256 B contiguous per
//      wave.  Only the one lane that owns the last, partial group of a row stores its 1..3 samples one by one.
// No sum's order depends on what else is in the launch or on how the utterance is cut into rows, and there are no atomics: the
// same input gives the same bits.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_out.h"

namespace itto {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

constexpr int WG = 256;
constexpr int PER = ITTO_RUN / WG;   // outputs per thread
constexpr int64_t MAX_INDEX = (int64_t)1 << 40;
static_assert(PER == 4, "a thread assembles four samples per store");

struct Params {
  const float* x;
  void* y;
  const float* kern_t;
  const itto_seg* segs;
  int64_t x_elems, y_elems;
  int orig, new_, width, taps, enc, run;
};

// Why a segment is refused (0: it is taken).  The entry point runs this on the host copy of the table and the kernel on the
// device copy: one statement of the range checks.
__host__ __device__ inline int seg_refusal(const itto_seg& g, int64_t x_elems, int64_t y_elems, int orig, int new_, int width) {
  if (g.x0 < 0 || g.n_in < 0 || g.x0 >= MAX_INDEX || g.n_in >= MAX_INDEX || g.N_total < -1 || g.N_total >= MAX_INDEX) return 1;
  if (g.j0 < 0 || g.j1 < g.j0 || g.j1 >= MAX_INDEX || g.j1 - g.j0 >= ((int64_t)1 << 30)) return 2;
  if (g.N_total >= 0 && (g.x0 + g.n_in > g.N_total || g.j1 > (g.N_total * new_ + orig - 1) / orig)) return 3;
  if (g.x_off < 0 || g.x_off + g.n_in > x_elems) return 4;
  if (g.y_off < 0 || (g.y_off & 3) != 0 || g.y_off + (g.j1 - g.j0) > y_elems) return 5;
  if (g.j1 > g.j0) {
    int64_t lo = (g.j0 / new_) * orig - width, hi = ((g.j1 - 1) / new_) * orig + width + orig;
    if (lo < 0) lo = 0;
    if (g.N_total >= 0 && hi > g.N_total) hi = g.N_total;
    if (lo < hi && (lo < g.x0 || hi > g.x0 + g.n_in)) return 6;
  }
  return 0;
}

// the int16 the PCM path has always produced: _vocode's clamp, then numpy's astype (truncation toward zero)
__device__ __forceinline__ int to_pcm16(float v) { return (int)fminf(fmaxf(v, -32767.f), 32767.f); }

// ITU-T G.711 mu-law: sign, 3-bit exponent, 4-bit mantissa of min(|s|, 32635) + 132, all bits inverted
__device__ __forceinline__ unsigned mulaw(int s) {
  const unsigned sign = s < 0 ? 0x80u : 0u;
  int mag = s < 0 ? -s : s;
  mag = (mag > 32635 ? 32635 : mag) + 132;                 // [132, 32767]: the leading one is bit 7 .. 14
  const int e = 24 - __builtin_clz((unsigned)mag);         // its position - 7
  return ~(sign | (unsigned)(e << 4) | (unsigned)((mag >> (e + 3)) & 15)) & 0xFFu;
}

// ITU-T G.711 A-law: the 13-bit value (s >> 3, a negative one in ones' complement), segment and mantissa, XOR 0x55 (0xD5 with
// the sign bit of a non-negative sample)
__device__ __forceinline__ unsigned alaw(int s) {
  int a = s >> 3;
  const unsigned mask = a >= 0 ? 0xD5u : 0x55u;
  a = a >= 0 ? a : ~a;                                      // [0, 4095]
  const int seg = a < 32 ? 0 : 27 - __builtin_clz((unsigned)a);
  return ((unsigned)(seg << 4) | (unsigned)((a >> (seg < 2 ? 1 : seg)) & 15)) ^ mask;
}

__global__ void __launch_bounds__(WG) pcm_out(Params p) {
  __shared__ __attribute__((aligned(16))) float s_x[ITTO_WINDOW];
  __shared__ __attribute__((aligned(16))) float s_v[ITTO_RUN];
  const int tid = threadIdx.x;
  const itto_seg sg = p.segs[blockIdx.y];
  // what the host checked on its copy of the table, again on the one this launch reads
  if (p.run < 4 || p.run > ITTO_RUN || (p.run & 3) != 0 || seg_refusal(sg, p.x_elems, p.y_elems, p.orig, p.new_, p.width)) return;
  const int64_t r0 = (int64_t)blockIdx.x * p.run;
  if (r0 >= sg.j1 - sg.j0) return;
  const int cnt = (int)min((int64_t)p.run, sg.j1 - sg.j0 - r0);
  const int ntap = p.kern_t ? p.taps : 1;                   // (24 kHz: one tap of weight 1 at the sample itself)
  const int64_t ja = sg.j0 + r0;
  const int64_t qa = ja / p.new_;
  const int pa = (int)(ja - qa * p.new_);
  const int span = ((pa + cnt - 1) / p.new_) * p.orig + ntap;
  if (span > ITTO_WINDOW) return;                           // (the entry point sizes `run` so that this cannot be)

  // 1. stage: sample i of the window is sample base + i of the utterance, which lies at x[x_off + base + i - x0]
  const float* x = p.x + sg.x_off;
  const int64_t base = qa * p.orig - p.width;
  for (int i = tid; i < span; i += WG) {
    const int64_t gi = base + i, li = gi - sg.x0;
    const bool inside = gi >= 0 && (sg.N_total < 0 || gi < sg.N_total) && li >= 0 && li < sg.n_in;
    s_x[i] = inside ? x[li] : 0.f;
  }
  __syncthreads();

  // 2. four chains per thread: output r = k * 256 + tid of the run has phase ph[k] and starts off[k] samples into the window
  int off[PER], ph[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = min(k * WG + tid, cnt - 1);               // (past the run's end: the last output again, never stored)
    const int dq = (pa + r) / p.new_;
    ph[k] = pa + r - dq * p.new_;
    off[k] = dq * p.orig;
  }
  float acc[PER] = {0.f, 0.f, 0.f, 0.f};
  if (p.kern_t) {
    const float* kt = p.kern_t;
    for (int t = 0; t < ntap; ++t, kt += p.new_) {
#pragma unroll
      for (int k = 0; k < PER; ++k) acc[k] = fmaf(kt[ph[k]], s_x[off[k] + t], acc[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = s_x[off[k]];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) s_v[k * WG + tid] = acc[k];
  __syncthreads();

  // 3. encode and store: four consecutive outputs per lane, one vector store
  const int r = PER * tid;
  if (r >= cnt) return;
  const int m = min(PER, cnt - r);
  const f32x4 v = *reinterpret_cast<const f32x4*>(s_v + r);
  const int64_t at = sg.y_off + r0 + r;                     // a multiple of 4: y_off and run are
  if (p.enc == ITTO_ENC_F32) {
    float* y = static_cast<float*>(p.y) + at;
    const f32x4 o = v * 0x1p-15f;
    if (m == PER) {
      *reinterpret_cast<f32x4*>(y) = o;
    } else {
      for (int i = 0; i < m; ++i) y[i] = o[i];
    }
    return;
  }
  int s[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) s[i] = to_pcm16(v[i]);
  if (p.enc == ITTO_ENC_PCM16) {
    int16_t* y = static_cast<int16_t*>(p.y) + at;
    if (m == PER) {
      i16x4 o = {(short)s[0], (short)s[1], (short)s[2], (short)s[3]};
      *reinterpret_cast<i16x4*>(y) = o;
    } else {
      for (int i = 0; i < m; ++i) y[i] = (int16_t)s[i];
    }
    return;
  }
  unsigned c[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) c[i] = p.enc == ITTO_ENC_MULAW ? mulaw(s[i]) : alaw(s[i]);
  uint8_t* y = static_cast<uint8_t*>(p.y) + at;
  if (m == PER) {
    *reinterpret_cast<uint32_t*>(y) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  } else {
    for (int i = 0; i < m; ++i) y[i] = (uint8_t)c[i];
  }
}

}  // namespace itto

#define ITTO_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      itto::set_error(__VA_ARGS__);  \
      return ITTO_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

extern "C" int itto_abi_version(void) { return ITTO_ABI_VERSION; }
extern "C" const char* itto_last_error(void) { return itto::g_err; }

extern "C" int itto_pcm_out(const itto_pcm_out_args* a, void* stream) {
  using namespace itto;
  ITTO_REQUIRE(a != nullptr, "itto_pcm_out: null argument struct");
  ITTO_REQUIRE(a->x && a->y && a->segs && a->segs_dev, "itto_pcm_out: null pointer");
  ITTO_REQUIRE(aligned(a->x, 4) && aligned(a->y, 16) && aligned(a->kern_t, 16) && aligned(a->segs_dev, 8),
               "itto_pcm_out: y and kern_t must be 16-byte aligned, segs_dev 8-byte aligned, x 4-byte aligned");
  ITTO_REQUIRE(a->n_seg >= 1 && a->n_seg <= 65535, "itto_pcm_out: n_seg must be 1..65535 (got %d)", a->n_seg);
  ITTO_REQUIRE(a->x_elems >= 0 && a->y_elems >= 0, "itto_pcm_out: negative element count");
  ITTO_REQUIRE(a->encoding >= ITTO_ENC_F32 && a->encoding <= ITTO_ENC_ALAW, "itto_pcm_out: encoding %d is none of ITTO_ENC_*", a->encoding);
  int run = ITTO_RUN;
  if (a->kern_t == nullptr) {
    ITTO_REQUIRE(a->orig == 1 && a->new_ == 1 && a->width == 0 && a->taps == 0,
                 "itto_pcm_out: without a tap table (kern_t NULL) orig = new = 1, width = taps = 0 (24 kHz: the encoding alone)");
  } else {
    ITTO_REQUIRE(a->orig >= 1 && a->orig <= ITTO_SRC_RATE && a->new_ >= 1 && a->width >= 1 && a->taps == 2 * (int64_t)a->width + a->orig,
                 "itto_pcm_out: taps must be 2 * width + orig (got orig=%d new=%d width=%d taps=%d)", a->orig, a->new_, a->width, a->taps);
    ITTO_REQUIRE((int64_t)a->new_ * a->taps * 4 <= ITTO_MAX_TAP_BYTES,
                 "itto_pcm_out: tap table of %lld bytes is above ITTO_MAX_TAP_BYTES = %d (new=%d taps=%d)",
                 (long long)a->new_ * a->taps * 4, ITTO_MAX_TAP_BYTES, a->new_, a->taps);
    ITTO_REQUIRE(4 * (int64_t)a->orig + a->taps <= ITTO_WINDOW,
                 "itto_pcm_out: 4 * orig + taps = %lld samples is above the staged window ITTO_WINDOW = %d (orig=%d taps=%d)",
                 4 * (long long)a->orig + a->taps, ITTO_WINDOW, a->orig, a->taps);
    // the longest run whose span, (1 + (run - 2) / new) * orig + taps at the most, fits the window
    while ((1 + (int64_t)(run - 2) / a->new_) * a->orig + a->taps > ITTO_WINDOW) run -= 4;
  }
  int64_t max_out = 0;
  for (int s = 0; s < a->n_seg; ++s) {
    const itto_seg& g = a->segs[s];
    switch (seg_refusal(g, a->x_elems, a->y_elems, a->orig, a->new_, a->width)) {
      case 0: break;
      case 1: ITTO_REQUIRE(false, "itto_pcm_out: segment %d: x0=%lld n_in=%lld N_total=%lld (x0, n_in >= 0; N_total >= 0 or -1)", s,
                           (long long)g.x0, (long long)g.n_in, (long long)g.N_total);
      case 2: ITTO_REQUIRE(false, "itto_pcm_out: segment %d: outputs [%lld, %lld) (0 <= j0 <= j1, fewer than 2^30)", s, (long long)g.j0, (long long)g.j1);
      case 3: ITTO_REQUIRE(false, "itto_pcm_out: segment %d reaches past the utterance's end: x0 + n_in = %lld, j1 = %lld, N_total = %lld", s,
                           (long long)(g.x0 + g.n_in), (long long)g.j1, (long long)g.N_total);
      case 4: ITTO_REQUIRE(false, "itto_pcm_out: segment %d lies outside x", s);
      case 5: ITTO_REQUIRE(false, "itto_pcm_out: segment %d lies outside y (y_off a multiple of 4, y_off + j1 - j0 <= y_elems)", s);
      default: ITTO_REQUIRE(false, "itto_pcm_out: segment %d: the support of the outputs [%lld, %lld) has not arrived (samples [%lld, %lld) are here)",
                            s, (long long)g.j0, (long long)g.j1, (long long)g.x0, (long long)(g.x0 + g.n_in));
    }
    if (g.j1 - g.j0 > max_out) max_out = g.j1 - g.j0;
  }
  if (max_out == 0) return ITTO_OK;                         // nothing to produce: no launch
  Params p;
  p.x = a->x, p.y = a->y, p.kern_t = a->kern_t, p.segs = a->segs_dev;
  p.x_elems = a->x_elems, p.y_elems = a->y_elems;
  p.orig = a->orig, p.new_ = a->new_, p.width = a->width, p.taps = a->taps, p.enc = a->encoding, p.run = run;
  dim3 grid((unsigned)((max_out + run - 1) / run), a->n_seg);
  hipLaunchKernelGGL(pcm_out, grid, dim3(WG), 0, static_cast<hipStream_t>(stream), p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("itto_pcm_out: %s", hipGetErrorString(e));
    return ITTO_ERR_LAUNCH;
  }
  return ITTO_OK;
}
