/*
 * indextts_fit.h -- C ABI of libindextts_fit.so: voice fitting on gfx950 (MI355X / CDNA4): the LoRA-specific gradient reduction
 * and the optimizer of IndexTTS.fit_voice (indextts/gpt/fit.py).
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

#define ITTF_ABI_VERSION 1

#define ITTF_F32 0
#define ITTF_BF16 1
#define ITTF_F16 2

#define ITTF_CHUNK 256   /* rows of one partial sum of ittf_lora_wgrad */
#define ITTF_MAX_RANK 64 /* the voice pool's own limit */
#define ITTF_SLICE 4096  /* elements one workgroup of ittf_sqnorm / ittf_adamw_step owns */

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

#ifdef __cplusplus
}
#endif
#endif
