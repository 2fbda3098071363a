/*
 * indextts_pitch.h -- C ABI of libindextts_pitch.so: resampling by an arbitrary ratio, every row at its own, on gfx950 (MI355X /
 * CDNA4).  It is the second step of the pitch shift (indextts/utils/tempo.py): WSOLA at the rate
 * speed / p (libindextts_tempo.so) changes the duration and keeps the pitch, this resampling by p brings the duration back to
 * 1 / speed and moves the pitch -- and the formants with it -- by the factor p.
 *
 * A library of its own, beside libindextts_hip.so, libindextts_voice.so, libindextts_audio.so, libindextts_out.so,
 * libindextts_post.so, libindextts_tempo.so, libindextts_codec.so and libindextts_score.so, whose ABIs it leaves alone: every name
 * here carries the prefix ittr_ / ITTR_.  Conventions as there: an entry point returns ITTR_OK (0) or an ITTR_ERR_* code, the
 * message is available from ittr_last_error() (thread-local); no exceptions cross the ABI, no hidden device allocations; a launch
 * is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default) and nothing synchronises with the host.
 *
 * The entry point takes the row table twice: in host memory, which it checks before it launches, and the same bytes in device
 * memory, which the kernel reads.  The kernel repeats the checks: it never reads or writes outside the element counts the args
 * struct states, whatever the device copy of the table holds.
 *
 * The computation, in integers (int64, ">>" an arithmetic shift) but for the weights and the sum.  A row has n >= 1 samples x,
 * xz[i] = x[i] for 0 <= i < n and 0 elsewhere; `step` is the ratio p as unsigned 32.32 fixed point (output m reads the input at
 * m p), `cutoff` the scale c of the filter's argument in units of 2^-16 (65536: the filter passes everything below the input's
 * Nyquist frequency; c < 1 for p > 1, where the cutoff lies at c / 2 of the input rate).  With HW = ITTR_HW, PH = ITTR_PHASES
 * = 2^8 and the table G of ITTR_TABLE fp32 values
 *     G[tap PH + phase] = h((tap PH + phase) / PH - HW),  h(u) = sinc(u) cos^2(pi u / (2 HW)) on |u| < HW, 0 elsewhere
 * (PH phases of 2 HW taps; h is 1 at 0 and 0 at the other integers exactly; G[2 HW PH ..] = 0 closes the table), output m of a
 * row is
 *     pos = m step;  i0 = pos >> 32;  f = pos - (i0 << 32)                 the read position m p = i0 + f / 2^32
 *     H   = (HW 65536 + cutoff - 1) / cutoff                               taps on either side: ceil(HW / c), 6 .. 12
 *     U_0 = ((f + ((H - 1) << 32)) cutoff >> 16) + (HW << 32)              c (m p - i) + HW for the first tap i = i0 - H + 1
 *     for j = 0 .. 2 H - 1, in this order:  i = i0 - H + 1 + j,  U = U_0 - j (cutoff << 16)      (exact: no position is a float)
 *       w_j = 0                                              if U < 0 or U >= 2 HW << 32
 *       w_j = fma(t, G[k + 1] - G[k], G[k]),  k = U >> 24,  t = (U mod 2^24) 2^-24  otherwise      the two phases, blended
 *       acc = fma(w_j, xz[i], acc)                                                                from acc = +0
 *     y[m] = acc (cutoff 2^-16)                                            the gain stays one: the taps are 1 / c apart in u
 * in fp32, one rounding per operation written.  At step = 2^32, cutoff = 65536 every weight is exactly 0 or 1: y = x, bit for bit.
 */
#ifndef INDEXTTS_PITCH_H
#define INDEXTTS_PITCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTR_OK 0
#define ITTR_ERR_INVALID 1 /* bad argument / refused table (nothing was launched) */
#define ITTR_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTR_ABI_VERSION 1

#define ITTR_HW 6           /* half-width of the windowed sinc in zero crossings: the one of the other resamplers */
#define ITTR_PHASES 256     /* phases per tap: the blend weight is the 24 bits below them */
#define ITTR_TABLE 3076     /* 2 HW PHASES values of h, then four zeros */
#define ITTR_CUTOFF_ONE 65536
#define ITTR_CUTOFF_MIN 32768                 /* c = 1/2: p = 2 */
#define ITTR_STEP_MIN 0x80000000ull           /* p = 1/2 */
#define ITTR_STEP_MAX 0x200000000ull          /* p = 2 */
#define ITTR_TILE 1024      /* consecutive outputs of one row a workgroup owns */

int ittr_abi_version(void);
const char* ittr_last_error(void);

/* One row: n samples at x + x_off, n_out outputs at y + y_off. */
typedef struct ittr_row {
  int64_t x_off;    /* elements of x; a multiple of 4 */
  int64_t n;        /* samples, 1 <= n < 2^30 */
  int64_t y_off;    /* elements of y; a multiple of 4 */
  int64_t n_out;    /* outputs, 1 <= n_out < 2^30 (the caller's choice: ceil(n 2^32 / step) reads no position past the row) */
  uint64_t step;    /* p in 32.32: ITTR_STEP_MIN .. ITTR_STEP_MAX */
  uint32_t cutoff;  /* c in 2^-16: ITTR_CUTOFF_MIN .. ITTR_CUTOFF_ONE */
  uint32_t reserved;
} ittr_row;

/* y[y_off + m] for 0 <= m < n_out of every row, nothing past them.  One workgroup owns ITTR_TILE consecutive outputs of ONE row:
 * it stages the table and the span of the row its outputs read in LDS; a lane sums its taps in the order above, without atomics.
 * Nothing depends on the row's place in the launch or on what else is in it: the same samples give the same bits.
 *   x        fp32 samples, 16-byte aligned
 *   y        fp32, 4-byte aligned, packed per row at y_off; may not overlap x
 *   table    fp32 [ITTR_TABLE] (device), 16-byte aligned
 *   rows     n_rows rows (1 <= n_rows <= 65535): x_off >= 0 and a multiple of 4, x_off + n <= x_elems; y_off >= 0 and a multiple
 *            of 4, y_off + n_out <= y_elems; n, n_out, step and cutoff in their ranges
 *   rows_dev 8-byte aligned */
typedef struct ittr_resample_ratio_args {
  const float* x;
  int64_t x_elems;
  float* y;
  int64_t y_elems;
  const float* table;
  int n_rows;
  int reserved;
  const ittr_row* rows;
  const ittr_row* rows_dev;
} ittr_resample_ratio_args;

int ittr_resample_ratio(const ittr_resample_ratio_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
