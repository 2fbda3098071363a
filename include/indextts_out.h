/*
 * indextts_out.h -- C ABI of libindextts_out.so: the gfx950 (MI355X / CDNA4) PCM output back-end
 * (indextts/utils/pcm_out.py): the vocoder's fp32 samples at 24 kHz -> any sample rate -> float,
 * PCM16 or G.711, for one utterance, a ragged batch of utterances or the rows of one stream boundary, in one launch.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), libindextts_voice.so (include/indextts_voice.h) and
 * libindextts_audio.so (include/indextts_audio.h), whose ABIs it leaves alone: every name here carries the prefix itto_ / ITTO_.
 * Conventions as there: an entry point returns ITTO_OK (0) or an ITTO_ERR_* code, the message is available from
 * itto_last_error() (thread-local); no exceptions cross the ABI, no hidden device allocations; the launch is asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = default) and nothing synchronises with the host.
 *
 * The entry point takes the segment table twice: `segs` in host memory, which it checks before it launches, and `segs_dev`, the
 * same bytes in device memory, which the kernel reads.  The kernel repeats the checks: it never reads or writes outside the
 * element counts the args struct states, whatever the device copy holds.
 */
#ifndef INDEXTTS_OUT_H
#define INDEXTTS_OUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTO_OK 0
#define ITTO_ERR_INVALID 1 /* bad argument / unsupported shape (nothing was launched) */
#define ITTO_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTO_ABI_VERSION 1

#define ITTO_SRC_RATE 24000          /* the vocoder's rate: orig = 24000 / g, new = rate / g */
#define ITTO_MAX_TAP_BYTES (1 << 20) /* a polyphase tap table [taps][new] fp32 may be this large */
#define ITTO_WINDOW 8192             /* fp32 input samples one workgroup stages: 4 * orig + taps must fit */
#define ITTO_RUN 1024                /* consecutive outputs of one row a workgroup owns, at most */

#define ITTO_ENC_F32 0   /* float:  v * 2^-15, nothing clamped                                   4 bytes per sample */
#define ITTO_ENC_PCM16 1 /* int16:  clamp to +-32767, truncate toward zero                       2 bytes per sample */
#define ITTO_ENC_MULAW 2 /* uint8:  ITU-T G.711 mu-law of that int16 (bias 132, clip 32635, inverted code byte) */
#define ITTO_ENC_ALAW 3  /* uint8:  ITU-T G.711 A-law of that int16 (13 bits, code XOR 0x55) */

int itto_abi_version(void);
const char* itto_last_error(void);

/* One row's piece of work.  The row is an utterance of N_total samples at 24 kHz (N_total == -1: its end is not known yet); the
 * launch holds its samples [x0, x0 + n_in) at x + x_off and produces its outputs j in [j0, j1) at y + y_off + (j - j0). */
typedef struct itto_seg {
  int64_t x_off;   /* elements of x */
  int64_t y_off;   /* elements of y (output samples); a multiple of 4 */
  int64_t x0;      /* the ABSOLUTE index within the utterance of the sample at x_off */
  int64_t n_in;    /* samples present */
  int64_t N_total; /* the utterance's length, or -1 while it is unknown */
  int64_t j0, j1;  /* the output indices to produce; j1 - j0 < 2^30 */
  int64_t reserved;
} itto_seg;

/* Polyphase sinc and encoding in one launch.  For j = q * new_ + p:
 *     v[j] = sum_{t < taps} kern[p][t] * x[q * orig + t - width],    x = 0 outside [0, N_total),
 *   one fp32 fmaf chain per output in ascending t, no atomics: the same input gives the same bits, whatever else is in the
 *   launch and however the utterance is cut into segments.  v then goes through `encoding` (ITTO_ENC_*).
 *   x        fp32 samples in the int16 range, as the vocoder leaves them
 *   y        float / int16_t / uint8_t by `encoding`; y_elems counts output samples
 *   kern_t   fp32 [taps][new_] (device): kern TRANSPOSED, so that the lanes of neighbouring phases read neighbouring addresses;
 *            taps == 2 * width + orig, at most ITTO_MAX_TAP_BYTES, 4 * orig + taps <= ITTO_WINDOW.  kern_t == NULL with
 *            orig == new_ == 1, width == 0, taps == 0 is the 24 kHz case: v = x.
 *   segs     n_seg pieces that share this tap table (1 <= n_seg <= 65535): x0 >= 0, n_in >= 0, j0 <= j1,
 *            N_total == -1 or N_total >= x0 + n_in (then j1 <= ceil(new_ * N_total / orig)),
 *            x_off + n_in <= x_elems, y_off + (j1 - j0) <= y_elems, y_off a multiple of 4,
 *            and the support of [j0, j1) is there: every input index i in [(j0 / new_) * orig - width,
 *            ((j1 - 1) / new_) * orig + width + orig) that lies in [0, N_total) -- in [0, inf) while the end is unknown --
 *            has x0 <= i < x0 + n_in.  A piece that asks for an output whose support has not arrived is refused.
 *   y and kern_t 16-byte aligned, segs_dev 8-byte aligned, x 4-byte aligned (a row may be a slice of a longer waveform) */
typedef struct itto_pcm_out_args {
  const float* x;
  int64_t x_elems;
  void* y;
  int64_t y_elems;
  const float* kern_t;
  int orig, new_, width, taps;
  int encoding;
  int n_seg;
  const itto_seg* segs;
  const itto_seg* segs_dev;
} itto_pcm_out_args;

int itto_pcm_out(const itto_pcm_out_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
