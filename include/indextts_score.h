/*
 * indextts_score.h -- C ABI of libindextts_score.so: likelihood scoring on gfx950 (MI355X / CDNA4): for every row of latents the
 * negative log-likelihood, the rank and the log-sum-exp of a GIVEN code under an output head, and the head's own best code, without
 * ever storing the [rows][vocabulary] logits (indextts/gpt/score.py).
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h), libindextts_voice.so (include/indextts_voice.h),
 * libindextts_audio.so (include/indextts_audio.h), libindextts_out.so (include/indextts_out.h), libindextts_post.so
 * (include/indextts_post.h), libindextts_tempo.so (include/indextts_tempo.h) and libindextts_codec.so (include/indextts_codec.h),
 * whose ABIs it leaves alone: every name here carries the prefix ittl_ / ITTL_.  Conventions as there: an entry point returns
 * ITTL_OK (0) or an ITTL_ERR_* code, the message is available from ittl_last_error() (thread-local); no exceptions cross the ABI,
 * no hidden device allocations; a launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default) and nothing
 * synchronises with the host.  Nothing is launched when an argument is refused.
 *
 * The quantities.  Row r is x [D] (fp32), the head is W [D][ldw] (row k at element k ldw; ldw >= V, a multiple of 8, is the pitch)
 * with the bias b [V] (fp32), the target is y in [0, V).  Two forms, chosen by `dtype`:
 *   ITTL_F32            W is fp32 and x is used as it is; D is a multiple of 4
 *   ITTL_BF16, ITTL_F16 W is bf16 / fp16, and x is rounded once (to nearest even) to that type when it is loaded; D is a multiple
 *                       of 8.  The products are exact in fp32 and the sum is fp32.
 *     l(j)  = (sum over k = 0 .. D - 1 of x[k] W[k][j], accumulated in fp32) + b[j]
 *     t     = l(y)                      (ittl_target_logit; ONE value of t serves both nll and rank)
 *     lse   = log sum over j of exp l(j)
 *     nll   = lse - t
 *     best  = the j of largest l(j); among equal logits the SMALLEST j
 *     rank  = the number of j != y with l(j) > t, or l(j) == t and j < y.  0: the target is the head's first choice; top-k accuracy
 *             for any k is rank < k.
 *   A row whose target lies outside [0, V) (-1 is the customary "ignore") gets nll = 0, t = 0, rank = -1; its lse and best are
 *   written all the same.  No kernel indexes with an unchecked target.  The columns V .. ldw - 1 of W never reach a result,
 *   whatever they hold (NaN included).
 *
 * THE ORDER OF THE SUMS.  Nothing below depends on the row's place in the launch, on n_rows or on the other rows: the same x, W,
 * b and y give the same bits of all five outputs in any batch and on every run.
 *   t:    l(y) by the very instructions, operand layout and k order that ittl_head_nll uses for l(j) (below), so t has the bits of
 *         the l(y) of that pass: a column that duplicates the target's compares EQUAL to t there and the tie rule decides.
 *   l(j): ITTL_F32: one chain from +0 in rising k, each term one fused multiply-add (v_mfma_f32_16x16x4_f32).
 *         16-bit: the matrix pipe's sum of 32 exact products at a time, k in rising blocks of 32 (v_mfma_f32_16x16x32_bf16 / _f16).
 *         Then + b[j].  K is zero-filled to the step (32 / 64): the extra terms are +0.
 *   lse:  a running pair (m, s), "the sum is s e^m", starts at (-inf, 0).  A logit v joins as
 *           v > m:  s = s E(m - v) + 1, m = v;      otherwise:  s = s + E(v - m)
 *         (a logit of -inf -- a column masked through its bias -- joins as nothing; a NaN logit makes the row's lse NaN)
 *         and two pairs join as  m = max(m1, m2),  s = s1 e1 + s2 e2,  ei = 1 if mi == m and E(mi - m) otherwise, every product and
 *         sum rounded on its own (no fused multiply-add).  E is the device's fast exponential (2^(v log2 e) on v_exp_f32).
 *         The columns are cut into ranges of ITTL_RANGE: range q is q ITTL_RANGE .. min(V, (q + 1) ITTL_RANGE) - 1.  Inside a range,
 *         with i = j - q ITTL_RANGE, column j goes to chain (h, c) = ((i >> 5) & 1, i & 15); a chain takes its columns in rising
 *         order.  The sixteen chains of one h join by pairs c with c ^ 1, then c ^ 2, c ^ 4, c ^ 8; then h = 0 joins h = 1; then
 *         the ranges join in rising q, one after the other from range 0.  lse = m + log s (the precise logf).
 *   rank: an integer count; best: the order (larger logit, then smaller j) is total on non-NaN logits, so neither depends on any
 *         order of evaluation.  A row whose logits are all NaN gets best = 0.
 */
#ifndef INDEXTTS_SCORE_H
#define INDEXTTS_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTL_OK 0
#define ITTL_ERR_INVALID 1 /* bad argument (nothing was launched) */
#define ITTL_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTL_ABI_VERSION 1

#define ITTL_RANGE 1024 /* consecutive columns one workgroup of ittl_head_nll streams */

#define ITTL_F32 0
#define ITTL_BF16 1
#define ITTL_F16 2

#define ITTL_WS_PER_ROW_RANGE 20 /* bytes of workspace per row and range: m, s, best logit (fp32), count, best id (int32) */

int ittl_abi_version(void);
const char* ittl_last_error(void);

/* t[r] = l(y[r]) of row r, or 0 where y[r] is outside [0, V): one gathered dot product per row.
 *   x        fp32 [n_rows][D], 16-byte aligned
 *   w        [D][ldw] of `dtype` (device), 16-byte aligned
 *   b        fp32 [V] (device), 4-byte aligned
 *   y        int32 [n_rows], 4-byte aligned
 *   t        fp32 [n_rows], 4-byte aligned; may not overlap x, w, b or y
 *   n_rows   1 <= n_rows < 2^31 - 64
 *   D        ITTL_F32: a multiple of 4 in 4 .. 65536; 16-bit: a multiple of 8 in 8 .. 65536
 *   V        1 <= V <= 2^24;  ldw: a multiple of 8, V <= ldw <= 2^24 + 8 */
typedef struct ittl_target_logit_args {
  const float* x;
  const void* w;
  const float* b;
  const int32_t* y;
  float* t;
  int64_t n_rows;
  int D, V, ldw;
  int dtype;
} ittl_target_logit_args;

int ittl_target_logit(const ittl_target_logit_args* a, void* stream);

/* nll, lse, best and rank of every row, see above, from x, W, b, y and the t that ittl_target_logit wrote.  The [n_rows][V]
 * logits are never stored: a workgroup owns 64 rows and one range of ITTL_RANGE columns and keeps, per row, the running (m, s),
 * the count of columns that beat t[r] and the best (logit, id).  With V > ITTL_RANGE the ranges' partial results go through `ws`
 * and meet in a second small launch, range by range in rising order, without atomics.
 *   x, w, b, y, n_rows, D, V, ldw, dtype   as for ittl_target_logit
 *   t        fp32 [n_rows] (read)
 *   nll, lse fp32 [n_rows]; best, rank  int32 [n_rows]; 4-byte aligned; none may overlap x, w, b, y, t or ws
 *   ws       ITTL_WS_PER_ROW_RANGE n_rows ceil(V / ITTL_RANGE) bytes, 16-byte aligned, when V > ITTL_RANGE (ws_bytes states its
 *            size); not touched otherwise.  May not overlap x, w, b, y or t. */
typedef struct ittl_head_nll_args {
  const float* x;
  const void* w;
  const float* b;
  const int32_t* y;
  const float* t;
  float* nll;
  float* lse;
  int32_t* best;
  int32_t* rank;
  void* ws;
  int64_t ws_bytes;
  int64_t n_rows;
  int D, V, ldw;
  int dtype;
} ittl_head_nll_args;

int ittl_head_nll(const ittl_head_nll_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
