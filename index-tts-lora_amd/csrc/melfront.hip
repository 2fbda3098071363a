// libindextts_audio.so (include/indextts_audio.h): the prompt audio front-end for gfx950 -- decoded waveform -> mono -> 24 kHz
// -> log-mel, two launches for any number of prompts (indextts/utils/audio_engine.py).
//
// resample_mean: one thread per output sample j = q * new + p of one wave: the channel mean of the taps' inputs formed on the
//   fly (the inputs of neighbouring outputs overlap and come from L1/L2), one fmaf chain over the phase's taps in ascending t.
// logmel: one workgroup (4 waves) per 16-frame tile of one prompt.
//   1. the tile's 16 * 256 + 768 samples are staged once in LDS, the reflection at either end of the prompt applied on the way;
//      a 256-sample block takes 264 floats, so that the 16 frames' float4 reads of one k land on 16 different bank quads
//   2. the windowed DFT is a GEMM [16 frames x 1024] x [1024 x 513] against a cosine and a sine basis on v_mfma_f32_16x16x4_f32
//      (exact fp32 fmaf-chain numerics).  A wave owns the 16-bin tiles nt = wave, wave + 4, ..; lane (r, g) reads the four
//      samples k = 16 ks + 4 g + j of frame r as one ds_read_b128 and the matching four basis values of bin 16 nt + r for cos and
//      for sin as one 16-byte load each (the host packs the basis in this order: every load of a wave is 1 KiB contiguous);
//      MFMA j reduces over the four k = 16 ks + 4 g + j, g = 0..3.  Re and im of a (frame, bin) are register i of the same lane
//      in two accumulators, so the magnitude is elementwise.  The basis comes from L2 / MALL behind a register double buffer
//      of eight k-steps (16 loads of 16 bytes): while the 64 MFMAs of one group run, the next group's loads are in flight
//      (s_waitcnt vmcnt counts down from 31 to 16 through a group in the compiled loop).
//   3. the magnitudes [16][513] go to LDS; thread (mel m, frame t) sums its bins [lo_m, hi_m) in ascending order, clips, takes
//      the log and stores to out + 100 * frame_off + m * T + t.
// No sum's order depends on what else is in the launch, and there are no atomics: the same input gives the same bits.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/indextts_audio.h"

namespace itta {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------------------------------------------- resample
constexpr int RS_WG = 256;

struct ResampleParams {
  const float* x;
  float* y;
  const float* kern;
  const itta_wave_seg* segs;
  int64_t x_elems, y_elems;
  int orig, new_, width, taps;
};

template <int C>
__device__ __forceinline__ float channel_mean(const float* x, int N, int i) {
  float s = x[i];
#pragma unroll
  for (int c = 1; c < C; ++c) s += x[(size_t)c * N + i];
  return C == 1 ? s : s / (float)C;
}
__device__ __forceinline__ float channel_mean_any(const float* x, int C, int N, int i) {
  float s = x[i];
  for (int c = 1; c < C; ++c) s += x[(size_t)c * N + i];
  return C == 1 ? s : s / (float)C;
}

__global__ void __launch_bounds__(RS_WG) resample_mean(ResampleParams p) {
  const itta_wave_seg sg = p.segs[blockIdx.y];
  const int j = blockIdx.x * RS_WG + threadIdx.x;
  // what the host checked on its copy of the table, again on the one this launch reads
  if (sg.C < 1 || sg.C > ITTA_MAX_CHANNELS || sg.N < 1 || sg.n_out < 0 || sg.x_off < 0 || sg.y_off < 0 ||
      sg.x_off + (int64_t)sg.C * sg.N > p.x_elems || sg.y_off + (int64_t)sg.n_out > p.y_elems)
    return;
  if (j >= sg.n_out) return;
  const float* x = p.x + sg.x_off;
  float acc;
  if (p.kern == nullptr) {
    acc = j < sg.N ? channel_mean_any(x, sg.C, sg.N, j) : 0.f;
  } else {
    const int q = j / p.new_, ph = j - q * p.new_;
    const float* k = p.kern + (size_t)ph * p.taps;
    const int64_t i0 = (int64_t)q * p.orig - p.width;
    int t0 = i0 < 0 ? (int)-i0 : 0;
    int64_t t1l = (int64_t)sg.N - i0;
    int t1 = t1l < p.taps ? (t1l < 0 ? 0 : (int)t1l) : p.taps;
    acc = 0.f;   // (a tap over a zero outside [0, N) would add +-0: skipping it leaves the same bits)
    if (sg.C == 1) {
      for (int t = t0; t < t1; ++t) acc = fmaf(k[t], channel_mean<1>(x, sg.N, (int)(i0 + t)), acc);
    } else if (sg.C == 2) {
      for (int t = t0; t < t1; ++t) acc = fmaf(k[t], channel_mean<2>(x, sg.N, (int)(i0 + t)), acc);
    } else {
      for (int t = t0; t < t1; ++t) acc = fmaf(k[t], channel_mean_any(x, sg.C, sg.N, (int)(i0 + t)), acc);
    }
  }
  p.y[sg.y_off + j] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ log-mel
constexpr int LM_WG = 256, LM_WAVES = LM_WG / 64;
constexpr int FT = 16;                                  // frames per tile
constexpr int TILE_SAMPLES = FT * ITTA_HOP + (ITTA_N_FFT - ITTA_HOP);   // 4864
constexpr int BLK_PAD = 8;                              // floats of padding per 256-sample block of the staged samples
constexpr int STAGE_FLOATS = TILE_SAMPLES + BLK_PAD * (TILE_SAMPLES / 256);   // 5016
constexpr int MAG_STRIDE = 545;                         // odd: the 16 frames of one bin fall on 16 banks
constexpr int KSTEPS = ITTA_N_FFT / 16;                 // 64 k-steps of 16
constexpr int PF = 8;                                   // k-steps per prefetch group
constexpr float LOG_FLOOR = -16.118095639f;             // log(1e-7f), rounded to fp32
static_assert(TILE_SAMPLES % 256 == 0 && KSTEPS % (2 * PF) == 0, "tile shape");

struct LogmelParams {
  const float* wave;
  float* out;
  const f32x4* basis;
  const float* fb_t;
  const int32_t* mel_rng;
  const itta_mel_seg* segs;
  int64_t wave_elems, out_elems;
  int n_seg;
};

__device__ __forceinline__ int staged(int i) { return i + BLK_PAD * (i >> 8); }

__device__ __forceinline__ void load_group(f32x4 (&b)[PF][2], const f32x4* bp, int ks) {
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    b[u][0] = bp[(size_t)(ks + u) * 128];
    b[u][1] = bp[(size_t)(ks + u) * 128 + 64];
  }
}
// The frame samples are the same for every bin tile, and left alone the compiler keeps all 64 float4 of a lane's frame in
// registers across the bin-tile loop -- 256 VGPRs, none left for the basis buffers, every basis load waited for at once.  The
// empty asm makes the row's offset opaque per group (the offset, not the pointer: a pointer through asm loses its LDS address
// space and the reads become flat loads): the four ds_read_b128 of a group stay with its MFMAs.
__device__ __forceinline__ void mma_group(const f32x4 (&b)[PF][2], const float* sx, int aoff, int ks, f32x4& re, f32x4& im) {
  asm volatile("" : "+v"(aoff));
  const float* arow = sx + aoff;
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int n = 16 * (ks + u);
    const f32x4 a = *reinterpret_cast<const f32x4*>(arow + n + BLK_PAD * (n >> 8));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      re = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[u][0][j], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[u][1][j], im, 0, 0, 0);
    }
  }
}

__global__ void __launch_bounds__(LM_WG) logmel(LogmelParams p) {
  __shared__ __attribute__((aligned(16))) float s_x[STAGE_FLOATS];
  __shared__ float s_mag[FT * MAG_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;

  // which prompt this tile belongs to: tiles are dealt prompt by prompt, ceil(T / 16) each
  int tile = blockIdx.x, s = 0;
  itta_mel_seg sg = p.segs[0];
  for (;;) {
    const int nt = sg.T > 0 ? (sg.T + FT - 1) / FT : 0;
    if (tile < nt) break;
    tile -= nt;
    if (++s >= p.n_seg) return;
    sg = p.segs[s];
  }
  const int N = sg.N, T = sg.T;
  // what the host checked on its copy of the table, again on the one this launch reads
  if (N <= ITTA_N_FFT / 2 || T != 1 + N / ITTA_HOP || sg.sample_off < 0 || sg.frame_off < 0 ||
      sg.sample_off + (int64_t)N > p.wave_elems || (int64_t)ITTA_N_MELS * (sg.frame_off + T) > p.out_elems)
    return;

  // 1. stage: sample i of the tile is sample (16 tile * 256 - 512 + i) of the centred, reflect-padded prompt
  const float* x = p.wave + sg.sample_off;
  const int first = tile * FT * ITTA_HOP - ITTA_N_FFT / 2;
  for (int i = tid; i < TILE_SAMPLES; i += LM_WG) {
    int src = first + i;
    if (src < 0) src = -src;
    if (src >= N) src = 2 * (N - 1) - src;
    s_x[staged(i)] = (src >= 0 && src < N) ? x[src] : 0.f;   // (past the reflection: only frames >= T read these)
  }
  __syncthreads();

  // 2. DFT: frame r of the tile starts at sample 256 r
  const int aoff = staged(256 * r) + 4 * g;
  for (int nt = wave; nt < ITTA_BIN_TILES; nt += LM_WAVES) {
    const f32x4* bp = p.basis + (size_t)nt * KSTEPS * 128 + lane;
    f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
    f32x4 b0[PF][2], b1[PF][2];
    load_group(b0, bp, 0);
#pragma unroll 1
    for (int ks = 0; ks < KSTEPS; ks += 2 * PF) {
      load_group(b1, bp, ks + PF);
      mma_group(b0, s_x, aoff, ks, re, im);
      load_group(b0, bp, min(ks + 2 * PF, KSTEPS - PF));   // (the last pass loads a group nobody uses: no branch in the loop)
      mma_group(b1, s_x, aoff, ks + PF, re, im);
    }
    // accumulator register i of lane (r, g): frame 4 g + i, bin 16 nt + r
    const int bin = 16 * nt + r;
    if (bin < ITTA_N_BINS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_mag[(4 * g + i) * MAG_STRIDE + bin] = sqrtf(fmaf(re[i], re[i], im[i] * im[i]));
    }
  }
  __syncthreads();

  // 3. mel, clip, log
  float* out = p.out + (int64_t)ITTA_N_MELS * sg.frame_off;
  for (int idx = tid; idx < FT * ITTA_N_MELS; idx += LM_WG) {
    const int t = idx & (FT - 1), m = idx >> 4;
    const int frame = tile * FT + t;
    if (frame >= T) continue;
    const int lo = max(0, p.mel_rng[2 * m]), hi = min((int)ITTA_N_BINS, p.mel_rng[2 * m + 1]);
    const float* w = p.fb_t + m * ITTA_N_BINS;
    const float* mg = s_mag + t * MAG_STRIDE;
    float acc = 0.f;
    for (int f = lo; f < hi; ++f) acc = fmaf(mg[f], w[f], acc);
    out[(int64_t)m * T + frame] = acc > 1e-7f ? logf(acc) : (acc == acc ? LOG_FLOOR : acc);   // (a NaN stays one, as in torch.clip)
  }
}

}  // namespace itta

#define ITTA_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      itta::set_error(__VA_ARGS__);  \
      return ITTA_ERR_INVALID;       \
    }                                \
  } while (0)

static bool aligned(const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; }

extern "C" int itta_abi_version(void) { return ITTA_ABI_VERSION; }
extern "C" const char* itta_last_error(void) { return itta::g_err; }

extern "C" int itta_resample(const itta_resample_args* a, void* stream) {
  using namespace itta;
  ITTA_REQUIRE(a != nullptr, "itta_resample: null argument struct");
  ITTA_REQUIRE(a->x && a->y && a->segs && a->segs_dev, "itta_resample: null pointer");
  ITTA_REQUIRE(aligned(a->x, 16) && aligned(a->y, 16) && aligned(a->kern, 16) && aligned(a->segs_dev, 8),
               "itta_resample: x, y and kern must be 16-byte aligned, segs_dev 8-byte aligned");
  ITTA_REQUIRE(a->n_seg >= 1 && a->n_seg <= 65535, "itta_resample: n_seg must be 1..65535 (got %d)", a->n_seg);
  ITTA_REQUIRE(a->x_elems >= 0 && a->y_elems >= 0, "itta_resample: negative element count");
  if (a->kern == nullptr) {
    ITTA_REQUIRE(a->orig == 1 && a->new_ == 1 && a->width == 0 && a->taps == 0,
                 "itta_resample: without a tap table (kern NULL) orig = new = 1, width = taps = 0 (the channel mean alone)");
  } else {
    ITTA_REQUIRE(a->orig >= 1 && a->new_ >= 1 && a->width >= 1 && a->taps == 2 * (int64_t)a->width + a->orig,
                 "itta_resample: taps must be 2 * width + orig (got orig=%d new=%d width=%d taps=%d)", a->orig, a->new_, a->width,
                 a->taps);
    ITTA_REQUIRE((int64_t)a->new_ * a->taps * 4 <= ITTA_MAX_TAP_BYTES,
                 "itta_resample: tap table of %lld bytes is above ITTA_MAX_TAP_BYTES = %d (new=%d taps=%d)",
                 (long long)a->new_ * a->taps * 4, ITTA_MAX_TAP_BYTES, a->new_, a->taps);
  }
  int max_out = 0;
  for (int s = 0; s < a->n_seg; ++s) {
    const itta_wave_seg& g = a->segs[s];
    ITTA_REQUIRE(g.C >= 1 && g.C <= ITTA_MAX_CHANNELS, "itta_resample: wave %d has C=%d channels (1..%d)", s, g.C, ITTA_MAX_CHANNELS);
    ITTA_REQUIRE(g.N >= 1, "itta_resample: wave %d has N=%d samples", s, g.N);
    const int64_t want = ((int64_t)a->new_ * g.N + a->orig - 1) / a->orig;
    ITTA_REQUIRE(want < ((int64_t)1 << 30) && g.n_out == want, "itta_resample: wave %d: n_out must be ceil(new * N / orig) = %lld (got %d)",
                 s, (long long)want, g.n_out);
    ITTA_REQUIRE(g.x_off >= 0 && g.x_off + (int64_t)g.C * g.N <= a->x_elems, "itta_resample: wave %d lies outside x", s);
    ITTA_REQUIRE(g.y_off >= 0 && g.y_off + (int64_t)g.n_out <= a->y_elems, "itta_resample: wave %d lies outside y", s);
    if (g.n_out > max_out) max_out = g.n_out;
  }
  ResampleParams p;
  p.x = a->x, p.y = a->y, p.kern = a->kern, p.segs = a->segs_dev;
  p.x_elems = a->x_elems, p.y_elems = a->y_elems;
  p.orig = a->orig, p.new_ = a->new_, p.width = a->width, p.taps = a->taps;
  dim3 grid((max_out + RS_WG - 1) / RS_WG, a->n_seg);
  hipLaunchKernelGGL(resample_mean, grid, dim3(RS_WG), 0, static_cast<hipStream_t>(stream), p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("itta_resample: %s", hipGetErrorString(e));
    return ITTA_ERR_LAUNCH;
  }
  return ITTA_OK;
}

extern "C" int itta_logmel(const itta_logmel_args* a, void* stream) {
  using namespace itta;
  ITTA_REQUIRE(a != nullptr, "itta_logmel: null argument struct");
  ITTA_REQUIRE(a->wave && a->out && a->basis && a->fb_t && a->mel_rng && a->segs && a->segs_dev, "itta_logmel: null pointer");
  ITTA_REQUIRE(aligned(a->wave, 16) && aligned(a->out, 16) && aligned(a->basis, 16) && aligned(a->fb_t, 16) &&
                   aligned(a->mel_rng, 8) && aligned(a->segs_dev, 8),
               "itta_logmel: wave, out, basis and fb_t must be 16-byte aligned, mel_rng and segs_dev 8-byte aligned");
  ITTA_REQUIRE(a->n_seg >= 1 && a->n_seg <= 65535, "itta_logmel: n_seg must be 1..65535 (got %d)", a->n_seg);
  ITTA_REQUIRE(a->wave_elems >= 0 && a->out_elems >= 0, "itta_logmel: negative element count");
  int64_t tiles = 0;
  for (int s = 0; s < a->n_seg; ++s) {
    const itta_mel_seg& g = a->segs[s];
    ITTA_REQUIRE(g.N > ITTA_N_FFT / 2, "itta_logmel: prompt %d has N=%d samples; the reflect padding needs N > %d", s, g.N,
                 ITTA_N_FFT / 2);
    ITTA_REQUIRE(g.N < (1 << 30) && g.T == 1 + g.N / ITTA_HOP, "itta_logmel: prompt %d: T must be 1 + N / 256 = %d (got %d)", s,
                 1 + g.N / ITTA_HOP, g.T);
    ITTA_REQUIRE(g.sample_off >= 0 && g.sample_off + (int64_t)g.N <= a->wave_elems, "itta_logmel: prompt %d lies outside wave", s);
    ITTA_REQUIRE(g.frame_off >= 0 && (int64_t)ITTA_N_MELS * (g.frame_off + g.T) <= a->out_elems, "itta_logmel: prompt %d lies outside out", s);
    tiles += (g.T + FT - 1) / FT;
  }
  ITTA_REQUIRE(tiles < ((int64_t)1 << 31), "itta_logmel: too many frame tiles");
  LogmelParams p;
  p.wave = a->wave, p.out = a->out, p.basis = reinterpret_cast<const f32x4*>(a->basis), p.fb_t = a->fb_t, p.mel_rng = a->mel_rng;
  p.segs = a->segs_dev, p.wave_elems = a->wave_elems, p.out_elems = a->out_elems, p.n_seg = a->n_seg;
  hipLaunchKernelGGL(logmel, dim3((unsigned)tiles), dim3(LM_WG), 0, static_cast<hipStream_t>(stream), p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("itta_logmel: %s", hipGetErrorString(e));
    return ITTA_ERR_LAUNCH;
  }
  return ITTA_OK;
}
