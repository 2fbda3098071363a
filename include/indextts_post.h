/*
 * indextts_post.h -- C ABI of libindextts_post.so: waveform finishing on gfx950 (MI355X / CDNA4) between the vocoder and the PCM
 * encoder (indextts/utils/post_wave.py): per-frame energy and peak of a ragged batch of utterances, and
 * one launch that gathers the pieces a host plan keeps of every utterance, fades them at the cuts and scales the row.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), libindextts_voice.so (include/indextts_voice.h),
 * libindextts_audio.so (include/indextts_audio.h) and libindextts_out.so (include/indextts_out.h), whose ABIs it leaves alone:
 * every name here carries the prefix ittp_ / ITTP_.  Conventions as there: an entry point returns ITTP_OK (0) or an ITTP_ERR_*
 * code, the message is available from ittp_last_error() (thread-local); no exceptions cross the ABI, no hidden device
 * allocations; a launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default) and nothing synchronises
 * with the host.
 *
 * An entry point takes each table twice: in host memory, which it checks before it launches, and the same bytes in device
 * memory, which the kernel reads.  The kernel repeats the checks: it never reads or writes outside the element counts the args
 * struct states, whatever the device copy holds.
 */
#ifndef INDEXTTS_POST_H
#define INDEXTTS_POST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTP_OK 0
#define ITTP_ERR_INVALID 1 /* bad argument / refused table (nothing was launched) */
#define ITTP_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTP_ABI_VERSION 1

#define ITTP_FRAME 240        /* samples per frame of ittp_frame_stats: 10 ms at 24 kHz */
#define ITTP_FADE 120         /* samples of the raised-cosine ramp at a cut: 5 ms */
#define ITTP_FRAMES_PER_WG 16 /* frames one workgroup of ittp_frame_stats covers (four per wave) */
#define ITTP_RUN 1024         /* consecutive outputs of one row a workgroup of ittp_splice owns */

int ittp_abi_version(void);
const char* ittp_last_error(void);

/* One utterance of ittp_frame_stats: n samples at x + x_off. */
typedef struct ittp_row {
  int64_t x_off; /* elements of x; a multiple of 4 (x is 16-byte aligned: every frame starts on a 16-byte boundary) */
  int64_t n;     /* samples, >= 1 */
} ittp_row;

/* Per-frame statistics of a ragged batch.  Row r has F_r = ceil(n_r / ITTP_FRAME) frames; frame f covers the samples
 * [f ITTP_FRAME, min((f + 1) ITTP_FRAME, n_r)) -- a sample beyond n_r counts as zero -- and writes two fp32 values,
 *     stats[2 (r stat_stride + f)]     = sum x^2
 *     stats[2 (r stat_stride + f) + 1] = max |x|
 *   (entries f >= F_r of a row are not written).
 *   The sum's order is fixed: lane l of ONE wave holds the frame's samples 4 l .. 4 l + 3 (l < 60; the lanes 60 .. 63 hold zeros)
 *   and forms p = x0 x0, p = fma(x1, x1, p), p = fma(x2, x2, p), p = fma(x3, x3, p); the 64 partial sums are then added pairwise
 *   across lane distances 32, 16, 8, 4, 2, 1.  Nothing in it depends on the frame's place in the launch, and there are no
 *   atomics: the same samples give the same bits.
 *   x        fp32 samples in the int16 range, as the vocoder leaves them; 16-byte aligned
 *   stats    fp32 [n_rows][stat_stride][2], 8-byte aligned; stats_elems counts floats
 *   rows     n_rows rows (1 <= n_rows <= 65535): x_off >= 0 and a multiple of 4, 1 <= n < 2^40, x_off + n <= x_elems,
 *            F_r <= stat_stride */
typedef struct ittp_frame_stats_args {
  const float* x;
  int64_t x_elems;
  float* stats;
  int64_t stats_elems;
  int64_t stat_stride;
  int n_rows;
  int reserved;
  const ittp_row* rows;
  const ittp_row* rows_dev;
} ittp_frame_stats_args;

int ittp_frame_stats(const ittp_frame_stats_args* a, void* stream);

/* One kept piece of a row: the source samples [src_off, src_off + n) of the row become its outputs [dst_off, dst_off + n). */
typedef struct ittp_piece {
  int64_t src_off;  /* samples from the row's first source sample */
  int64_t dst_off;  /* samples from the row's first output */
  int64_t n;        /* >= fade_in + fade_out */
  int32_t fade_in;  /* 0, or ITTP_FADE: the piece starts at a cut and rises over its first ITTP_FADE samples */
  int32_t fade_out; /* 0, or ITTP_FADE: the piece ends at a cut and falls over its last ITTP_FADE samples */
} ittp_piece;

/* One output row of ittp_splice: n_in source samples at x + x_off, n_out outputs at y + y_off, assembled from the pieces
 * [piece0, piece0 + n_pieces) of the piece table, every output scaled by `gain`. */
typedef struct ittp_out_row {
  int64_t x_off;    /* elements of x */
  int64_t n_in;     /* source samples of the row */
  int64_t y_off;    /* elements of y; a multiple of 4 */
  int64_t n_out;    /* outputs of the row: the sum of its pieces' n */
  int32_t piece0;   /* index of the row's first piece */
  int32_t n_pieces; /* >= 0 */
  float gain;       /* finite */
  int32_t reserved;
} ittp_out_row;

/* Gather, fade and scale in one launch.  For output j of a row, in piece k at i = j - dst_off_k:
 *     y[y_off + j] = (gain * w) * x[x_off + src_off_k + i],   two fp32 multiplies, in this order,
 *     w = ramp[i] for i < fade_in, ramp[n_k - 1 - i] for n_k - 1 - i < fade_out, 1 elsewhere
 *   (so gain 1 without a fade copies the bits, and a power of two scales exactly).  One workgroup owns ITTP_RUN consecutive
 *   outputs of ONE row and every output has one source sample: a row's bits do not depend on what else is in the launch.
 *   x        fp32 samples, 4-byte aligned
 *   y        fp32, 16-byte aligned, packed per row at y_off
 *   ramp     fp32 [ITTP_FADE] (device): the raised-cosine ramp, computed in float64 by the caller and rounded once to fp32
 *   rows     n_rows rows (1 <= n_rows <= 65535): x_off, n_in, n_out >= 0, below 2^40; x_off + n_in <= x_elems; y_off >= 0, a
 *            multiple of 4, y_off + n_out <= y_elems; piece0 + n_pieces <= n_pieces of the table; gain finite
 *   pieces   n_pieces pieces.  A piece outside its source row (src_off < 0 or src_off + n > n_in) is refused; so is one whose
 *            fades are neither 0 nor ITTP_FADE or with n < fade_in + fade_out; the pieces of a row are in output order and tile
 *            [0, n_out): one that starts before its predecessor ends overlaps it and is refused, and so is a gap.
 *   rows_dev 8-byte aligned, pieces_dev 8-byte aligned */
typedef struct ittp_splice_args {
  const float* x;
  int64_t x_elems;
  float* y;
  int64_t y_elems;
  const float* ramp;
  int n_rows;
  int n_pieces;
  const ittp_out_row* rows;
  const ittp_out_row* rows_dev;
  const ittp_piece* pieces;
  const ittp_piece* pieces_dev;
} ittp_splice_args;

int ittp_splice(const ittp_splice_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
