/*
 * indextts_tempo.h -- C ABI of libindextts_tempo.so: the speaking rate on gfx950 (MI355X / CDNA4), between the vocoder and waveform
 * finishing (indextts/utils/tempo.py): WSOLA time-scale modification of a ragged batch of utterances at
 * 24 kHz, every row at its own speed.  Pitch and formants stay; only the duration changes.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), libindextts_voice.so (include/indextts_voice.h),
 * libindextts_audio.so (include/indextts_audio.h), libindextts_out.so (include/indextts_out.h) and libindextts_post.so
 * (include/indextts_post.h), whose ABIs it leaves alone: every name here carries the prefix ittm_ / ITTM_.  Conventions as
 * there: an entry point returns ITTM_OK (0) or an ITTM_ERR_* code, the message is available from ittm_last_error()
 * (thread-local); no exceptions cross the ABI, no hidden device allocations; a launch is asynchronous on `stream` (a hipStream_t
 * passed as void*; NULL = default) and nothing synchronises with the host.
 *
 * An entry point takes the row table twice: in host memory, which it checks before it launches, and the same bytes in device
 * memory, which the kernel reads.  The kernel repeats the checks: it never reads or writes outside the element counts the args
 * struct states, whatever the device copies of the table and of the offsets hold.
 *
 * The algorithm, in integers (int64) but for the sums.  For a row of n >= 1 samples x at the speed S / 1024, with
 * xz[i] = x[i] for 0 <= i < n and 0 elsewhere:
 *     n_out = max(1, (n 1024 + S / 2) / S)                          outputs                        ("/" rounds down)
 *     K     = (n_out - 1) / HOP + 2                                 frames
 *     a_k   = (k HOP S + 512) / 1024 - HOP                          the nominal start of frame k in x
 *     p_0   = a_0 = -HOP, d_0 = 0;  for k = 1 .. K - 1:
 *       t[i] = xz[p_(k-1) + HOP + i], i < WIN                       the template: how the previous choice goes on
 *       c(d) = sum_(i < WIN) t[i] xz[a_k + d + i],  -TOL <= d < TOL the score of a lag
 *       d_k  = the lag of largest c; among equal scores the one of smallest |d|, and of +-d the negative one;  p_k = a_k + d_k
 *     y[m]  = w[HOP + j] xz[p_k0 + HOP + j] + w[j] xz[p_(k0+1) + j],  j = m mod HOP, k0 = m / HOP, 0 <= m < n_out
 *     w[i]  = 1/2 - 1/2 cos(2 pi i / WIN)                           computed in float64 by the caller, rounded once to fp32
 */
#ifndef INDEXTTS_TEMPO_H
#define INDEXTTS_TEMPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTM_OK 0
#define ITTM_ERR_INVALID 1 /* bad argument / refused table (nothing was launched) */
#define ITTM_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTM_ABI_VERSION 1

#define ITTM_HOP 384       /* synthesis hop: 16 ms at 24 kHz */
#define ITTM_WIN 768       /* window and template: 32 ms */
#define ITTM_TOL 192       /* the lags are -ITTM_TOL .. ITTM_TOL - 1: 384 of them */
#define ITTM_SPEED_ONE 1024 /* S of speed 1 */
#define ITTM_SPEED_MIN 512  /* speed 0.5 */
#define ITTM_SPEED_MAX 2048 /* speed 2 */
#define ITTM_RUN 1024      /* consecutive outputs of one row a workgroup of ittm_overlap_add owns */

int ittm_abi_version(void);
const char* ittm_last_error(void);

/* One utterance: n samples at x + x_off at the speed `speed` / 1024; its K lags at offsets + o_off, its n_out outputs at
 * y + y_off.  The same table serves both launches (ittm_search does not look at y_off). */
typedef struct ittm_row {
  int64_t x_off;    /* elements of x; a multiple of 4 */
  int64_t n;        /* samples, 1 <= n < 2^40 */
  int64_t o_off;    /* elements of offsets; a multiple of 4 */
  int64_t y_off;    /* elements of y; a multiple of 4 */
  int32_t speed;    /* S: ITTM_SPEED_MIN .. ITTM_SPEED_MAX */
  int32_t reserved;
} ittm_row;

/* The chain of lags d_0 = 0, d_1 .. d_(K-1) of every row: offsets[o_off + k] = d_k (int32); nothing is written past a row's K
 * entries.  A row's chain is sequential -- the template of frame k is where the choice of frame k - 1 goes on -- so ONE
 * workgroup walks it; the rows of a launch are independent workgroups, without atomics and without a word between them.
 *   The sum of one lag has a fixed order: four partial sums, partial q over the terms i = q, q + 4, q + 8, ... in rising order,
 *   each term added with one fma (s_q = fma(t[i], xz[a_k + d + i], s_q), from +0), and c = (s_0 + s_1) + (s_2 + s_3).  Nothing
 *   in it depends on the row's place in the launch: the same samples give the same bits, and the same lags.
 *   x        fp32 samples (finite), 16-byte aligned
 *   offsets  int32, 4-byte aligned
 *   rows     n_rows rows (1 <= n_rows <= 65535): x_off >= 0 and a multiple of 4, 1 <= n < 2^40, x_off + n <= x_elems; speed in
 *            [ITTM_SPEED_MIN, ITTM_SPEED_MAX]; o_off >= 0 and a multiple of 4, o_off + K <= offsets_elems
 *   rows_dev 8-byte aligned */
typedef struct ittm_search_args {
  const float* x;
  int64_t x_elems;
  int32_t* offsets;
  int64_t offsets_elems;
  int n_rows;
  int reserved;
  const ittm_row* rows;
  const ittm_row* rows_dev;
} ittm_search_args;

int ittm_search(const ittm_search_args* a, void* stream);

/* The outputs of every row from its samples and its lags: y[y_off + m] for 0 <= m < n_out, nothing past them,
 *     y = fma(w[j], xz[p_(k0+1) + j], w[HOP + j] * xz[p_k0 + HOP + j])      one fp32 multiply, then one fma.
 *   One workgroup owns ITTM_RUN consecutive outputs of ONE row: a row's bits do not depend on what else is in the launch.  A lag
 *   of any value is taken (a sample outside the row is zero): the kernel reads no sample outside [x_off, x_off + n).
 *   x        fp32 samples, 4-byte aligned
 *   offsets  int32, 4-byte aligned: what ittm_search wrote for the same table
 *   y        fp32, 16-byte aligned, packed per row at y_off; may not overlap x
 *   window   fp32 [ITTM_WIN] (device), 16-byte aligned
 *   rows     as ittm_search, and y_off >= 0 and a multiple of 4, y_off + n_out <= y_elems */
typedef struct ittm_overlap_add_args {
  const float* x;
  int64_t x_elems;
  const int32_t* offsets;
  int64_t offsets_elems;
  float* y;
  int64_t y_elems;
  const float* window;
  int n_rows;
  int reserved;
  const ittm_row* rows;
  const ittm_row* rows_dev;
} ittm_overlap_add_args;

int ittm_overlap_add(const ittm_overlap_add_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
