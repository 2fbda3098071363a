/*
 * indextts_fit.h -- C ABI of libindextts_fit.so: voice fitting on gfx950 (MI355X / CDNA4): the LoRA-specific gradient reduction,
 * the optimizer and the ragged causal training attention, forward and backward, of IndexTTS.fit_voice (indextts/gpt/fit.py,
 * DESIGN.md sections 4.29 and 4.30).
 *
 * A library of its own, beside libindextts_hip.so (include/indextts_hip.h) and the eight others (include/indextts_voice.h,
 * _audio.h, _out.h, _post.h, _tempo.h, _codec.h, _score.h, _pitch.h), whose ABIs it leaves alone: every name here carries the
 * prefix ittf_ / ITTF_.  Conventions as there: an entry point returns ITTF_OK (0) or an ITTF_ERR_* code, the message is available
 * from ittf_last_error() (thread-local); no exceptions cross the ABI, no hidden device allocations; a launch is asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = default) and nothing synchronises with the host.  Nothing is launched when an
 * argument is refused.  No kernel uses an atomic: the same operands give the same bits on every run.
 *
 * THE FACTOR GRADIENT (ittf_lora_wgrad).  One form behind both factors of y = x W + b + scale (x A^T) B^T:
 *     G[j][c] = (accumulate ? G[j][c] : 0) + scale * sum over m = 0 .. M - 1 of s[m][j] z[m][c],    j < r, c < C
 *   dB^T = u^T dy:  s = u [M][r], z = dy [M][N];   dA = du^T x:  s = du [M][r], z = x [M][K].
 *   s, z row-major with the leading dimensions lds >= r, ldz >= C (elements), so the [x | u] operand is read in place; rows >= M of
 *   either buffer are never read.  dtype: ITTF_F32 (v_mfma_f32_16x16x4_f32) or ITTF_BF16 / ITTF_F16 (v_mfma_f32_16x16x32_*: the
 *   products are exact in fp32); the sums are fp32.
 *   THE ORDER OF THE SUM.  The rows are cut into chunks of ITTF_CHUNK: chunk q is rows q ITTF_CHUNK .. min(M, (q + 1) ITTF_CHUNK)
 *   - 1.  Inside a chunk one accumulator per (j, c) from +0 takes the rows in rising steps of 4 (fp32) or 32 (16-bit) rows, one
 *   matrix instruction per step (rows past M are +0 terms).  The chunks' partial sums go through `ws` and a second launch adds
 *   them from +0 in rising q, multiplies by scale and then adds the old G when `accumulate` is set; each of the three is rounded
 *   on its own.  Nothing depends on the launch geometry or on the run.
 *
 * THE OPTIMIZER (ittf_sqnorm, ittf_adamw_step).  Both walk a TABLE of parameter segments on the device (ittf_segment, n_seg of
 * them; the caller built it and answers for its pointers and lengths: `start` is the sum of the lengths in front of a segment and
 * `total` the sum of all).  The elements of all segments, in table order, are cut into slices of ITTF_SLICE; a workgroup owns a
 * slice.
 *   ittf_sqnorm: out[0] = sum of g^2 over every element.  Thread t of a slice's workgroup adds its elements t, t + 256, ... in
 *     rising order from +0 (fused multiply-add), the 256 threads meet in a binary tree (t with t + 128, then + 64, ... + 1), the
 *     slices' sums lie in `ws` and one workgroup adds them the same way (thread t takes slices t, t + 256, ...).
 *   ittf_adamw_step, per element, with g' = clip * g, group G = segment's group (0 or 1), every operation fp32 and rounded on its
 *     own, in this order (torch.optim.AdamW's):
 *         p  = p * (1 - lr[G] * wd[G])
 *         m  = m + (g' - m) * (1 - beta1)
 *         v  = v * beta2 + (1 - beta2) * g' * g'          (fused: v beta2 rounded, then fma(g' (1 - beta2), g', .))
 *         p  = p - (lr[G] / bc1) * ( m / (sqrt(v) / bc2_sqrt + eps) )
 *     bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) are the host's.  Then t_copy = p rounded ONCE to `dtype` (a copy for
 *     ITTF_F32) where the segment has a t_copy: same element order as p.  Nothing past a segment's n elements is touched.
 *
 * THE TRAINING ATTENTION (ittf_attn_fwd, ittf_attn_bwd).  Causal softmax attention over RAGGED rows: fp32 in, fp32 sums
 * (v_mfma_f32_16x16x4_f32) and fp32 out whatever the engine's dtype, head dimension 64, read in place from the fp32 output of the
 * attn.c_attn GEMM:  qkv [M][ld], D = 64 H; q of head h at column 64 h + e, k at D + 64 h + e, v at 2 D + 64 h + e.
 *     s[i][j] = scale * sum_e q[i][e] k[j][e]  (j <= i, rows of one segment),   lse[i] = ln sum_j exp(s[i][j]),
 *     p[i][j] = exp(s[i][j] - lse[i]),   out[i][d] = sum_j p[i][j] v[j][d]                 out [M][ldo], head h at column 64 h + d
 *     dP[i][j] = sum_d dout[i][d] v[j][d],   delta[i] = sum_j p[i][j] dP[i][j],   ds[i][j] = p[i][j] (dP[i][j] - delta[i])
 *     dq[i] = scale sum_j ds[i][j] k[j],   dk[j] = scale sum_i ds[i][j] q[i],   dv[j] = sum_i p[i][j] dout[i]
 *   dqkv [M][ld] has qkv's layout; lse is [H][M].  The backward recomputes p from qkv and lse tile by tile: nothing of size [n][n]
 *   is stored anywhere.  delta is sum_d dout[i][d] out[i][d] in exact arithmetic; it is formed as sum_j p dP, from the bits of p
 *   and dP that ds is then formed from, because ds is a difference of nearly equal numbers wherever one key holds a row's whole
 *   weight, and rowsum(dout o out) carries the rounding of out into it (dq of such a row missed its bound
 *   fourfold).  The backward therefore does not read out.
 *   RAGGED ROWS.  A table of n_seg records ittf_rows (first row, row count) on the device, which the caller built and answers for
 *   (the host cannot see it): the segments come in rising order, do not overlap, lie inside [0, M), and none is longer than
 *   max_len, the longest the caller states (at most ITTF_ATTN_MAX_SEG).  A segment is one utterance: its rows attend causally to
 *   rows of the same segment only, and it may start at any row.  Rows of M that no segment covers are never read and never
 *   written, in any operand.  (A kernel cuts a record at max_len rows and at row M, so that a wrong table cannot reach outside the
 *   operands.)
 *   OWNERSHIP.  Every output tile has one owner and no workgroup waits for another: a wave owns 16 query rows of one (segment,
 *   head) in the forward (out, lse) and in the dq launch, and 16 key rows in the dk / dv launch; the backward is two launches (dq,
 *   whose first sweep leaves delta in `ws`; then dk and dv) and computes the scores three times.
 *   THE ORDER OF THE SUMS.  Rows are counted from the segment's first row; tile t is rows 16 t .. 16 t + 15; rows past the
 *   segment's end are +0 operands.  Nothing below depends on the segment's place in M, on the other segments, on ld, ldo or on
 *   the launch.  A "chain" is one accumulator through successive matrix instructions, each adding 4 products to it.
 *     a score, or sum_d dout[i][d] v[j][d]: a chain of 16 over the 64 columns, instruction 4 a + b taking columns 16 a + b + 4 c,
 *       c = 0 .. 3; the chain starts from +0.
 *     forward, per query row, over the key tiles 0 .. its own in rising order (online softmax): s = scale * score rounded once;
 *       the tile's maximum joins the running maximum m (alpha = exp(m_old - m_new), 0 before the first tile);
 *       p = exp(s - m_new) (0 above the diagonal); the tile's sum of p is ((p0 + p1) + p2) + p3 over the keys 4 c + 0 .. 3 of each
 *       c, then (c = 0 with 1) + (c = 2 with 3);  l = fma(l, alpha, that sum);  every out accumulator is multiplied by alpha and
 *       then takes a chain of 4 over the tile, instruction b taking keys b, 4 + b, 8 + b, 12 + b.  At the end out = acc / l and
 *       lse = m + ln l.
 *     backward: s = scale * score rounded once (the forward's bits), p = exp(s - lse[i]).  delta[i]: for each c = 0 .. 3 one
 *       fma chain from +0 over the key tiles 0 .. i's own in rising order, inside a tile over the keys 4 c + 0 .. 3, of p dP; then
 *       (c = 0 with 1) + (c = 2 with 3).  ds' = p * (dP - delta[i]).  dv[j] and dk[j] take the query tiles
 *       from j's own upward, dq[i] the key tiles 0 .. i's own, each a chain of 4 per tile (instruction b: rows b, 4 + b, 8 + b,
 *       12 + b of the tile) into one accumulator from +0; dq and dk are multiplied by scale once at the end.
 */
#ifndef INDEXTTS_FIT_H
#define INDEXTTS_FIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTF_OK 0
#define ITTF_ERR_INVALID 1 /* bad argument (nothing was launched) */
#define ITTF_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTF_ABI_VERSION 2

#define ITTF_F32 0
#define ITTF_BF16 1
#define ITTF_F16 2

#define ITTF_CHUNK 256   /* rows of one partial sum of ittf_lora_wgrad */
#define ITTF_MAX_RANK 64 /* the voice pool's own limit */
#define ITTF_SLICE 4096  /* elements one workgroup of ittf_sqnorm / ittf_adamw_step owns */
#define ITTF_ATTN_MAX_SEG 4096   /* the longest segment (rows) ittf_attn_fwd / ittf_attn_bwd take */
#define ITTF_ATTN_MAX_HEADS 256  /* heads of 64 columns */
#define ITTF_ATTN_MAX_NSEG 65535 /* records of a row table */

int ittf_abi_version(void);
const char* ittf_last_error(void);

/* bytes of workspace ittf_lora_wgrad needs for M rows, rank r and C columns: 4 ceil(M / ITTF_CHUNK) 16 ceil(r / 16) C (0 when an
 * argument is out of range) */
int64_t ittf_wgrad_ws_bytes(int64_t M, int r, int C);

/* G, see above.
 *   s        [M][lds] of `dtype`, element-aligned (device);  z  [M][ldz] likewise
 *   G        fp32 [r][ldg], 4-byte aligned; may not overlap s, z or ws
 *   ws       ittf_wgrad_ws_bytes(M, r, C) bytes, 16-byte aligned (ws_bytes states its size)
 *   M        1 <= M < 2^31 - ITTF_CHUNK;  r  1 .. ITTF_MAX_RANK;  C  1 .. 2^24
 *   lds >= r, ldz >= C, ldg >= C, each at most 2^24 + 64 */
typedef struct ittf_lora_wgrad_args {
  const void* s;
  const void* z;
  float* G;
  void* ws;
  int64_t ws_bytes;
  int64_t M;
  int r, C;
  int lds, ldz, ldg;
  int dtype;
  int accumulate;
  float scale;
} ittf_lora_wgrad_args;

int ittf_lora_wgrad(const ittf_lora_wgrad_args* a, void* stream);

/* one parameter segment (64 bytes): n elements of the fp32 master p, its gradient g, the moments m and v, and the copy t_copy in
 * the step's dtype (NULL: none); start = the number of elements in the segments in front of it; group 0 or 1 */
typedef struct ittf_segment {
  float* p;
  const float* g;
  float* m;
  float* v;
  void* t_copy;
  int64_t n;
  int64_t start;
  int32_t group;
  int32_t reserved;
} ittf_segment;

/* floats of workspace ittf_sqnorm needs for `total` elements: ceil(total / ITTF_SLICE) */
int64_t ittf_sqnorm_ws_floats(int64_t total);

/* out[0] = the sum of g^2 over the table, see above.
 *   table    ittf_segment [n_seg] on the device, 16-byte aligned; 1 <= n_seg <= 65536; 1 <= total < 2^40
 *   ws       fp32 [ittf_sqnorm_ws_floats(total)], 4-byte aligned (ws_floats states its size);  out  fp32 [1], 4-byte aligned */
int ittf_sqnorm(const ittf_segment* table, int n_seg, int64_t total, float* ws, int64_t ws_floats, float* out, void* stream);

/* one AdamW step over the table, see above.  lr, wd: per group; beta1, beta2 in [0, 1); eps > 0; bc1, bc2_sqrt in (0, 1];
 * clip in [0, 1]; dtype of the t_copy buffers.  The scalars are doubles: what the kernel multiplies by -- 1 - lr wd, lr / bc1, 1 - beta1,
 * beta2, 1 - beta2, bc2_sqrt, eps, clip -- is formed in double here and rounded to fp32 once. */
typedef struct ittf_adamw_args {
  const ittf_segment* table;
  int n_seg;
  int dtype;
  int64_t total;
  double lr[2];
  double wd[2];
  double beta1, beta2, eps;
  double bc1, bc2_sqrt;
  double clip;
} ittf_adamw_args;

int ittf_adamw_step(const ittf_adamw_args* a, void* stream);

/* one segment of rows (16 bytes): rows first .. first + count - 1 of the [M]-row operands */
typedef struct ittf_rows {
  int64_t first;
  int64_t count;
} ittf_rows;

/* bytes of workspace ittf_attn_bwd needs for M rows of H heads: 4 H M, the delta of every (head, row) (0 when an argument is out of
 * range) */
int64_t ittf_attn_ws_bytes(int64_t M, int H);

/* the training attention, see above.  One struct for both entry points; ittf_attn_fwd ignores dout, dqkv, ws and ws_bytes,
 * ittf_attn_bwd ignores out (it may be NULL there; ldo is dout's pitch).
 *   qkv      fp32 [M][ld] (device), 16-byte aligned, ld >= 3 * 64 H and a multiple of 4
 *   out      fp32 [M][ldo], 16-byte aligned, ldo >= 64 H and a multiple of 4: written by fwd
 *   lse      fp32 [H][M], 4-byte aligned: written by fwd, read by bwd
 *   dout     fp32 [M][ldo] (out's pitch), 16-byte aligned;  dqkv  fp32 [M][ld] (qkv's pitch), 16-byte aligned: written by bwd
 *   ws       ittf_attn_ws_bytes(M, H) bytes, 4-byte aligned (ws_bytes states its size)
 *   table    ittf_rows [n_seg] on the device, 16-byte aligned; 1 <= n_seg <= ITTF_ATTN_MAX_NSEG
 *   max_len  the longest segment of the table, 1 .. ITTF_ATTN_MAX_SEG;  M  1 <= M < 2^31;  H  1 .. ITTF_ATTN_MAX_HEADS
 *   ld, ldo  at most 2^24 + 64;  scale  finite and > 0
 * What a call writes (fwd: out, lse; bwd: dqkv, ws) may not overlap anything else it is given. */
typedef struct ittf_attn_args {
  const float* qkv;
  float* out;
  float* lse;
  const float* dout;
  float* dqkv;
  void* ws;
  int64_t ws_bytes;
  const ittf_rows* table;
  int64_t M;
  int n_seg;
  int max_len;
  int H;
  int ld, ldo;
  float scale;
} ittf_attn_args;

int ittf_attn_fwd(const ittf_attn_args* a, void* stream);
int ittf_attn_bwd(const ittf_attn_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
