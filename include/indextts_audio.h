/*
 * indextts_audio.h -- C ABI of libindextts_audio.so: the gfx950 (MI355X / CDNA4) prompt audio front-end
 * (indextts/utils/audio_engine.py): decoded waveform -> mono -> 24 kHz -> log-mel [100][T], for one
 * prompt or a ragged batch of prompts, in two launches.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h) and libindextts_voice.so (include/indextts_voice.h),
 * whose ABIs it leaves alone: every name here carries the prefix itta_ / ITTA_.  Conventions as there: an entry point returns
 * ITTA_OK (0) or an ITTA_ERR_* code, the message is available from itta_last_error() (thread-local); no exceptions cross the
 * ABI, no hidden device allocations; a launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default) and
 * nothing synchronises with the host.
 *
 * Both entry points take a segment table twice: `segs` in host memory, which the entry point checks before it launches, and
 * `segs_dev`, the same bytes in device memory, which the kernel reads.  A kernel never reads or writes outside the element
 * counts the args struct states, whatever the device copy holds.
 */
#ifndef INDEXTTS_AUDIO_H
#define INDEXTTS_AUDIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTA_OK 0
#define ITTA_ERR_INVALID 1 /* bad argument / unsupported shape (nothing was launched) */
#define ITTA_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTA_ABI_VERSION 1

#define ITTA_MAX_CHANNELS 8
#define ITTA_MAX_TAP_BYTES (1 << 20) /* a polyphase tap table [new][taps] fp32 may be this large */

#define ITTA_N_FFT 1024
#define ITTA_HOP 256
#define ITTA_N_BINS 513
#define ITTA_N_MELS 100
#define ITTA_BIN_TILES 33 /* ceil(513 / 16): the basis is packed for this many 16-bin tiles, zeros past bin 512 */
/* fp32 elements of the packed basis: [ITTA_BIN_TILES][64 k-steps][2: cos, sin][64 lanes][4] */
#define ITTA_BASIS_ELEMS (ITTA_BIN_TILES * 64 * 2 * 64 * 4)

int itta_abi_version(void);
const char* itta_last_error(void);

/* One wave of a resample launch: planar fp32 x[C][N] at x + x_off, its mono 24 kHz form y[n_out] at y + y_off,
 * n_out = ceil(new * N / orig). */
typedef struct itta_wave_seg {
  int64_t x_off; /* elements */
  int64_t y_off; /* elements */
  int32_t C, N;
  int32_t n_out;
  int32_t reserved;
} itta_wave_seg;

/* Channel mean and polyphase sinc in one launch.  For j = q * new_ + p:
 *     y[j] = sum_{t < taps} kern[p][t] * xbar[q * orig + t - width],    xbar = 0 outside [0, N),
 *   xbar[i] = (x[0][i] + x[1][i] + .. + x[C-1][i]) / C  in fp32, summed in channel order; one fp32 fmaf chain per output in
 *   ascending t, no atomics: the same input gives the same bits.
 *   kern     fp32 [new_][taps] (device), taps == 2 * width + orig, at most ITTA_MAX_TAP_BYTES.  kern == NULL with
 *            orig == new_ == 1, width == 0, taps == 0 is the 24 kHz case: the launch writes the channel mean alone.
 *   segs     n_seg waves that share this tap table (1 <= n_seg <= 65535); C in [1, ITTA_MAX_CHANNELS], N >= 1,
 *            x_off + C * N <= x_elems, y_off + n_out <= y_elems
 *   x, y, kern 16-byte aligned, segs_dev 8-byte aligned */
typedef struct itta_resample_args {
  const float* x;
  int64_t x_elems;
  float* y;
  int64_t y_elems;
  const float* kern;
  int orig, new_, width, taps;
  const itta_wave_seg* segs;
  const itta_wave_seg* segs_dev;
  int n_seg;
} itta_resample_args;

int itta_resample(const itta_resample_args* a, void* stream);

/* One prompt of a log-mel launch: N samples at wave + sample_off, T = 1 + N / 256 frames, its mel [100][T] contiguous at
 * out + 100 * frame_off. */
typedef struct itta_mel_seg {
  int64_t sample_off; /* elements */
  int64_t frame_off;  /* frames */
  int32_t N, T;
} itta_mel_seg;

/* Framing (n_fft 1024, hop 256, centred, reflect padding of 512: index -i -> i, N-1+i -> N-1-i), windowed DFT, magnitude,
 * mel and log(max(., 1e-7)) in one launch.  A workgroup owns 16 consecutive frames of ONE prompt: a prompt's mel in a batch
 * is bit-equal to the same prompt alone.
 *   basis    fp32 [ITTA_BASIS_ELEMS] (device): element (((nt * 64 + ks) * 2 + cs) * 64 + 16 g + c) * 4 + j holds
 *            window[k] * (cs ? sin : cos)(2 pi k f / 1024),  k = 16 ks + 4 g + j,  f = 16 nt + c  (zero for f > 512)
 *   fb_t     fp32 [100][513] (device): the mel filterbank, transposed
 *   mel_rng  int32 [100][2] (device): mel m sums the bins [lo_m, hi_m) in ascending order
 *   segs     n_seg prompts (1 <= n_seg <= 65535); N > 512 (the reflection needs it), T == 1 + N / 256,
 *            sample_off + N <= wave_elems, 100 * (frame_off + T) <= out_elems
 *   wave, out, basis, fb_t 16-byte aligned, mel_rng and segs_dev 8-byte aligned */
typedef struct itta_logmel_args {
  const float* wave;
  int64_t wave_elems;
  float* out;
  int64_t out_elems;
  const float* basis;
  const float* fb_t;
  const int32_t* mel_rng;
  const itta_mel_seg* segs;
  const itta_mel_seg* segs_dev;
  int n_seg;
} itta_logmel_args;

int itta_logmel(const itta_logmel_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
