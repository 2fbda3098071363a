/*
 * indextts_codec.h -- C ABI of libindextts_codec.so: the acoustic tokenizer on gfx950 (MI355X / CDNA4): a log-mel [100, T] to the
 * 8192-entry mel codes of the decoder, with the encoder half of the DVAE (indextts/vqvae/dvae.py).  fp32
 * throughout: the result is a discrete decision per frame.
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), libindextts_voice.so (include/indextts_voice.h),
 * libindextts_audio.so (include/indextts_audio.h), libindextts_out.so (include/indextts_out.h), libindextts_post.so
 * (include/indextts_post.h) and libindextts_tempo.so (include/indextts_tempo.h), whose ABIs it leaves alone: every name here
 * carries the prefix ittc_ / ITTC_.  Conventions as there: an entry point returns ITTC_OK (0) or an ITTC_ERR_* code, the message
 * is available from ittc_last_error() (thread-local); no exceptions cross the ABI, no hidden device allocations; a launch is
 * asynchronous on `stream` (a hipStream_t passed as void*; NULL = default) and nothing synchronises with the host.
 *
 * ittc_conv takes the segment table twice: in host memory, which it checks before it launches, and the same bytes in device
 * memory, which the kernel reads.  The kernel repeats the checks: it never reads or writes outside the row counts the args
 * struct states, whatever the device copy of the table holds.
 *
 * The algorithm.  All operands are channels-last: a tensor of R rows and C channels is fp32 [R][C], row r at element r C.
 *
 *   The convolution of one clip (a segment): x_len >= 1 input rows, taps in {1, 3}, stride in {1, 2}, pad = (taps - 1) / 2,
 *   y_len = (x_len + stride - 1) / stride output rows.  With xz[i] = the clip's row i for 0 <= i < x_len and 0 elsewhere (never
 *   the neighbouring clip's rows), in(v) = max(v, 0) under ITTC_RELU_IN and v otherwise:
 *     acc(t, o) = sum over k = 0 .. K - 1 of in(xz[t stride + tap - pad][c]) W[k][o],     k = tap Cin + c,  K = taps Cin
 *   THE ORDER OF THE SUM: one chain from +0 in rising k -- tap 0 with its channels 0 .. Cin - 1 first, then tap 1, then tap 2 --
 *   every term added with one fused multiply-add, acc = fma(in(x), W[k][o], acc).  (The packed weights are zero-padded to
 *   Kpad = K rounded up to a multiple of ITTC_KSTEP; the padding terms are fma(0, 0, acc) and change nothing.)  Then
 *     v = acc + bias[o];   v = v + resid[t][o] under ITTC_RESIDUAL;   y[t][o] = max(v, 0) under ITTC_RELU_OUT, v otherwise.
 *   Nothing in it depends on the clip's place in the launch or on the other clips: the same inputs give the same bits in any
 *   batch and on every run.
 *
 *   The packed weights of a torch conv1d weight w [Cout][Cin][taps]:  W[tap Cin + c][o] = w[o][c][tap], fp32 [Kpad][Cout], rows
 *   K .. Kpad - 1 zero.  The caller packs once.
 *
 *   The nearest code of a row z [D] in a codebook e [D][J] (column j is code j):
 *     s(j) = (sum over k = 0 .. D - 1 of z[k] e[k][j], one fma chain from +0 in rising k) - h[j],    h[j] = |e_j|^2 / 2
 *     code = the j of largest s(j); among equal scores the SMALLEST j.
 *   h is computed by the caller in float64 and rounded once to fp32.  argmax s = argmin |z - e_j|^2: the term |z|^2 is common to
 *   every j and is left out.  The comparison (larger score, then smaller j) is a total order on finite scores, so neither the
 *   split of the codes over workgroups nor the pairing inside one changes the result.
 */
#ifndef INDEXTTS_CODEC_H
#define INDEXTTS_CODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTC_OK 0
#define ITTC_ERR_INVALID 1 /* bad argument / refused table (nothing was launched) */
#define ITTC_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTC_ABI_VERSION 1

#define ITTC_KSTEP 32        /* the packed K is a multiple of this */
#define ITTC_CODE_RANGE 1024 /* consecutive codes one workgroup of ittc_nearest_code searches */

#define ITTC_RELU_IN 1  /* max(x, 0) on the input operand */
#define ITTC_RELU_OUT 2 /* max(v, 0) on the output */
#define ITTC_RESIDUAL 4 /* + resid before the output ReLU */

int ittc_abi_version(void);
const char* ittc_last_error(void);

/* One clip: its x_len input rows start at row x_row0 of x, its y_len output rows at row y_row0 of y (and of resid). */
typedef struct ittc_seg {
  int64_t x_row0;
  int64_t x_len; /* 1 <= x_len < 2^31 */
  int64_t y_row0;
  int64_t reserved;
} ittc_seg;

/* y = conv(x) over n_seg clips, see above.  Rows of y outside every clip's y_len rows are not written; the clips' output rows
 * must not overlap each other (not checked: it would only be the caller's own race).
 *   x        fp32 [x_rows][Cin], 16-byte aligned; Cin a multiple of 4
 *   w        packed weights fp32 [Kpad][Cout] (device), 16-byte aligned; w_elems = Kpad Cout states which pack it is and is
 *            checked against taps, Cin and Cout
 *   bias     fp32 [Cout] (device), 16-byte aligned
 *   resid    fp32 [y_rows][Cout], 16-byte aligned, under ITTC_RESIDUAL; NULL otherwise
 *   y        fp32 [y_rows][Cout], 16-byte aligned; Cout a multiple of 4; may not overlap x or resid
 *   segs     n_seg clips (1 <= n_seg <= 65535): x_row0 >= 0, x_row0 + x_len <= x_rows; y_row0 >= 0, y_row0 + y_len <= y_rows
 *   segs_dev 8-byte aligned */
typedef struct ittc_conv_args {
  const float* x;
  int64_t x_rows;
  const float* w;
  int64_t w_elems;
  const float* bias;
  const float* resid;
  float* y;
  int64_t y_rows;
  int Cin, Cout;
  int taps, stride;
  int flags;
  int n_seg;
  const ittc_seg* segs;
  const ittc_seg* segs_dev;
} ittc_conv_args;

int ittc_conv(const ittc_conv_args* a, void* stream);

/* code[r] = the nearest code of row r of z, for 0 <= r < n_rows, see above; score[r] = its s, if score is not NULL.
 * The [n_rows][J] scores are never stored: a workgroup keeps a running (score, code) per row over its ITTC_CODE_RANGE codes.
 * With J > ITTC_CODE_RANGE the ranges' winners go through `ws` and meet in a second small launch, range by range in rising
 * order, without atomics.
 *   z        fp32 [n_rows][D] (finite), 16-byte aligned; D a multiple of 4, 4 <= D <= 65536
 *   embed    fp32 [D][J] (device), 16-byte aligned; J a multiple of 4, 4 <= J <= 2^24
 *   h        fp32 [J] (device), 16-byte aligned
 *   code     int32 [n_rows], 4-byte aligned
 *   score    fp32 [n_rows] or NULL
 *   ws       8 n_rows ceil(J / ITTC_CODE_RANGE) bytes, 16-byte aligned, when J > ITTC_CODE_RANGE (ws_bytes states its size);
 *            not read otherwise
 *   n_rows   1 <= n_rows < 2^31 - 64 */
typedef struct ittc_nearest_code_args {
  const float* z;
  const float* embed;
  const float* h;
  int32_t* code;
  float* score;
  void* ws;
  int64_t ws_bytes;
  int64_t n_rows;
  int D, J;
} ittc_nearest_code_args;

int ittc_nearest_code(const ittc_nearest_code_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
