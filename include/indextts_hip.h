/*
 * indextts_hip.h -- C ABI of libindextts_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the IndexTTS
 * inference hot path (GPT-2 acoustic-token decoder with KV cache + conditioned BigVGAN vocoder).
 *
 * Conventions
 *   - every entry point returns ITTS_OK (0) or an ITTS_ERR_* code; the message is available from
 *     itts_last_error() (thread-local).  No exceptions cross the ABI, no hidden device allocations: all
 *     buffers (outputs, workspaces) are passed in by the caller.  Launches are asynchronous on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream) and are hipGraph-capturable.
 *   - `dtype` selects the storage type T of weights / T-typed activations: ITTS_F32, ITTS_BF16, ITTS_F16.
 *     All accumulation is fp32.  The GPT residual stream, logits and LayerNorm statistics are always fp32.
 *   - activations of the vocoder are channels-last: [B][T][C] (time-major rows, channels contiguous).
 *
 * Reference interfaces replaced (paths relative to the reference repo, CreateIntelligens/index-tts-lora):
 *   itts_aa_snake_fwd      <- the reference's only native op: anti_alias_activation_cuda.forward(input, up_filter,
 *                             down_filter, alpha, beta), indextts/BigVGAN/alias_free_activation/cuda/
 *                             anti_alias_activation.cpp:19-22 / anti_alias_activation_cuda.cu:44-181,214-256, and its
 *                             torch twin alias_free_torch/act.py:10-28 (the numerical oracle).
 *   itts_gemm_skinny,
 *   itts_ln_reduce,
 *   itts_attn_decode,
 *   itts_embed_step,
 *   itts_sample            <- one cached decode step of GPT2InferenceModel.forward (indextts/gpt/model.py:163-193)
 *                             + the HF generate() logits processors / token selection reached from model.py:710-715.
 *   itts_gemm_conv,
 *   itts_attn_prefill,
 *   itts_layernorm         <- prefill branch (model.py:151-162) and the teacher-forced latent pass
 *                             UnifiedVoice.forward(return_latent=True) (model.py:548-597, 459-474).
 *   itts_gemm_conv,
 *   itts_aa_snake_fwd,
 *   itts_tanh_pcm          <- BigVGAN.forward / AMPBlock1.forward (indextts/BigVGAN/models.py:203-252, 65-74) and the
 *                             output stage of IndexTTS.infer (indextts/infer.py:892-893).
 */
#ifndef INDEXTTS_HIP_H
#define INDEXTTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTS_OK 0
#define ITTS_ERR_INVALID 1 /* bad argument / unsupported shape (nothing was launched) */
#define ITTS_ERR_LAUNCH 2  /* HIP reported an error at launch */

#define ITTS_F32 0
#define ITTS_BF16 1
#define ITTS_F16 2

#define ITTS_ABI_VERSION 10 /* 10: one header and one argument struct per launch family -- itts_skinny_args gains w_scale (itts_gemm_skinny_w8 takes that struct), itts_sample_args gains rows (itts_sample_rows takes that struct), itts_lora_shrink_args gains mix (itts_lora_shrink_mix takes that struct), the three near-copy structs of those entry points are gone; no symbol was renamed or removed; 9: itts_last_kernel (read-only: the kernel form the last itts_gemm_conv / itts_aa_snake_fwd launched), itts_lora_shrink (a new symbol: no existing struct or signature changed), and itts_sample_rows; 8: prompt front-end (itts_subsample_conv, itts_mha_small, itts_glu_dwconv_ln_silu, itts_rows, itts_geglu, itts_prefix_rows) and speaker encoder (itts_im2col_reflect, itts_res2_step, itts_se_gate, itts_scale_resid, itts_col_stats, ITTS_EPI_RELU_AFFINE_*), itts_kv_share_rows, ITTS_EPI_SILU_STORE, y_row0 / y_mtp and any M with rows_per_wg in itts_gemm_skinny, itts_gemm_conv ksplit <= 64; 7: LayerNorm folded into the consuming skinny GEMM (ln_c), residual epilogue with a packed T copy, rows_per_wg / wide_wg, bump words in itts_gemm_skinny / itts_embed_step (+ clamp, packed copy); the reducer tail is gone; paged KV cache (kv_tab / kv_bs); 6: per-row clocks (row_step0) in itts_embed_step / itts_sample_args (slot refill), itts_attn_prefill_prefix / _shared, kv_share in itts_attn_decode; 5: itts_ln_reduce takes up to 6 slabs */

int itts_abi_version(void);
const char* itts_last_error(void);
/* The kernel form (and its template parameters) that the calling thread's last itts_gemm_conv or itts_aa_snake_fwd call
 * launched, e.g. "conv_narrow_lds<f16,96,7,1,8,30>" or "aa_snake_mfma<3,pair>"; "" if that call launched nothing.
 * Thread-local like itts_last_error; a static string set by the launch site itself (no effect on what is launched). */
const char* itts_last_kernel(void);
/* The product library keeps no process-wide mutable state besides these thread-local strings and immutable tables:
 * tuning overrides and in-kernel time stamps exist only in the diagnostic build (include/indextts_hip_diag.h). */

/* ------------------------------------------------------------------------------------------------------------------
 * Packed weight layout (shared by itts_gemm_skinny and itts_gemm_conv).  A logical matrix W[K][N] (K = reduction
 * dim, N = output columns) is stored as 1-KiB blocks in MFMA B-fragment order:
 *     block(nt, ks) , nt = n/16 in [0, ceil(N/16)), ks = k/KS in [0, ceil(K/KS)),  KS = 32 (bf16/f16) or 16 (f32)
 *     inside a block: lane l = (g<<4)|c (g = 0..3, c = 0..15) owns 16 contiguous bytes = E elements
 *                     W[ks*KS + g*E + e][nt*16 + c],  e = 0..E-1,  E = 8 (bf16/f16) or 4 (f32)
 *     block order: ((tap * NT + nt) * KT + ks), zero-padded in K and N.
 * itts_pack_weight performs this packing on the device.
 * ------------------------------------------------------------------------------------------------------------------ */
int itts_pack_weight(const void* w /* [taps][K][N] T, row-major */, void* packed, int taps, int K, int N, int dtype,
                     void* stream);
/* bytes needed for `packed` */
int64_t itts_packed_bytes(int taps, int K, int N, int dtype);

/* ------------------------------------------------------------------------------------------------------------------
 * Anti-aliased periodic activation (Activation1d(SnakeBeta)):
 *   replicate-pad 5 | x2 zero-stuffed 12-tap FIR (gain 2) | x + sin^2(x e^alpha)/(e^beta + 1e-9) | replicate-pad 5/6
 *   | 12-tap stride-2 FIR.   alpha/beta are the log-scale per-channel parameters; fp32 accumulation.
 * layout 0: x,y are [B][T][C] (channels-last, product path);  layout 1: [B][C][T] (the reference op's layout).
 * valid_rows (layout 0 only, NULL = all T rows): int32 [B] on the device, the length of each batch element's sequence --
 * the filters' replicate padding clamps there, as if the element were processed alone; rows past it are not written.
 * ------------------------------------------------------------------------------------------------------------------ */
int itts_aa_snake_fwd(const void* x, void* y, const float* alpha_log, const float* beta_log, const float* up_filter12,
                      const float* down_filter12, int B, int T, int C, int dtype, int layout, const int32_t* valid_rows,
                      void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Packed activation layout of the decode step (optional, per operand).  A T-typed activation matrix X[M][K] that a skinny
 * GEMM consumes can be stored in MFMA-fragment order, 1 KiB per (k-step, 16-row tile):
 *     element (m, k) at  ((k / KS * MTP + m / 16) * 64 + (k % KS) / E * 16 + m % 16) * E + k % E,   MTP = ceil(M / 16),
 *     KS = 32, E = 8 (bf16/f16) or KS = 16, E = 4 (f32); the buffer holds K/KS * MTP KiB (rows up to 16*MTP exist).
 * The GEMM then reads a fragment as one contiguous 1-KiB wave-load instead of 16 rows x 64 bytes.  Producers that can
 * write it: itts_ln_reduce (y_packed), itts_attn_decode (out_packed), itts_gemm_skinny (y_packed), itts_embed_step (h_packed).
 * ------------------------------------------------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------------------------------------------------
 * Paged KV cache (optional, per call: kv_tab != NULL).  The contiguous cache of one layer is T [rows][H][smax][64].  The paged
 * form is a pool T [blocks][H][kv_bs][64], kv_bs in {16, 32, 64} positions per block, plus a block table int32
 * [rows][ITTS_KV_TAB] on the device: position j of cache row r lives in block kv_tab[r][(j / kv_bs) % ITTS_KV_TAB], offset
 * j % kv_bs.  The table is a RING over the position index: the decode loop's shared write position only grows, a row's live
 * window [pad_r, pos] must stay under (ITTS_KV_TAB - 2) * kv_bs positions, and the caller (GPTEngine) deals blocks to rows as
 * the loop advances and takes them back when a row has stopped -- a refilled decode slot reclaims the blocks of the row that
 * left.  Every table entry must always name a block of the pool (rows past their window point at a scratch block): the
 * kernels read clamped / masked positions without branching.  `smax` is ignored in the paged form.
 * Entry points that take (kv_tab, kv_bs): itts_gemm_skinny (QKV epilogue: append), itts_attn_decode, itts_attn_prefill_packed /
 * _prefix / _shared (prompt rows in, cached prefix out).  Beam search keeps the contiguous form (its per-position row table).
 * ------------------------------------------------------------------------------------------------------------------ */
#define ITTS_KV_TAB 64

/* ------------------------------------------------------------------------------------------------------------------
 * Skinny GEMM for the decode step: Y[M][N] = epi( X[M][K] @ W[K][N] + bias ), up to 96 rows (bf16/f16; 16 in fp32) per
 * pass over the weights (larger M is processed in row chunks by the entry point, or -- rows_per_wg > 0 -- as ONE launch
 * whose row tiles are dealt to grid.z: the prompt front-end's ~150-row GEMMs).  1-3 16-column tiles (x one K slice)
 * per workgroup, the K range split over the workgroup's waves and reduced deterministically through LDS; every global
 * load is issued before its first use (one memory round trip per launch); 8/16-byte epilogue accesses.
 * ------------------------------------------------------------------------------------------------------------------ */
#define ITTS_EPI_STORE 0      /* y (T [M][N]) = v */
#define ITTS_EPI_GELU_STORE 1 /* y (T [M][N]) = gelu_new(v) */
#define ITTS_EPI_RESID_F32 2  /* yf (fp32 [M][N]) += v   (residual stream update; ksplit 1: one owner per element); if y != NULL
                                 the new values are also stored as T in y ([M][N], or packed with y_packed) */
#define ITTS_EPI_QKV_CACHE 3  /* cols [0,D): y (T [M][D]) = v ; [D,2D): K cache ; [2D,3D): V cache, at position *pos */
#define ITTS_EPI_STORE_F32 4  /* yf (fp32 [M][N]) = v               (logits) */
#define ITTS_EPI_SLAB_F32 5   /* yf (fp32 [ksplit][M][N]): slice ks stores its partial product (bias added by slice 0);
                                 the slabs are summed in order by itts_ln_reduce */
#define ITTS_EPI_SILU_STORE 6 /* y (T [M][N]) = v * sigmoid(v)   (the Conformer's feed-forward activation) */
#define ITTS_EPI_RELU_AFFINE_STORE 7      /* y (T) = relu(v) * post_scale[n] + post_shift[n]: a TDNN block of the speaker encoder,
                                             eval-mode BatchNorm behind the ReLU (indextts/BigVGAN/ECAPA_TDNN.py:79-130) */
#define ITTS_EPI_RELU_AFFINE_TANH_STORE 8 /* y (T) = tanh(relu(v) * post_scale[n] + post_shift[n])  (the attention branch of its pooling) */

typedef struct itts_skinny_args {
  int dtype;
  int M, N, K;
  const void* wp;    /* packed W */
  const float* bias; /* [N] or NULL */
  const void* x;     /* T [M][K] */
  int epi;
  void* y;
  float* yf;
  void* kcache; /* T [M][heads][smax][64] for this layer */
  void* vcache;
  const int32_t* pos; /* device scalar: cache row to write */
  int heads, smax;
  int ksplit; /* split-K over workgroups (grid.y); > 1 only with ITTS_EPI_SLAB_F32 */
  /* LayerNorm folded into this GEMM (ln_c != NULL; bf16 / f16, ksplit 1, N % 4 == 0, storing epilogues):
   *     v = rstd[m] * ( (x @ wp)[m][n] - mean[m] * ln_c[n] ) + bias[n]
   * with mean / rstd the LayerNorm statistics (eps = ln_eps, 0 = 1e-5) of row m of x itself, computed by the kernel from the
   * operand fragments.  For wp = pack(gamma . W), ln_c[n] = sum_k (gamma . W)[k][n] (of the T-rounded values),
   * bias[n] = sum_k beta[k] W[k][n] + b[n] this equals LN(x; gamma, beta) @ W + b: HF GPT2Block's ln_1 -> c_attn and
   * ln_2 -> c_fc (indextts/gpt/model.py:163-193) without a LayerNorm launch in front of the GEMM. */
  const float* ln_c;
  float ln_eps;
  int32_t* bump; /* device word incremented once by the launch, or NULL (the decode loop's step counter: a launch that does
                    not read it advances it) */
  /* geometry hints (results differ only in the summation order): rows_per_wg 0 = every workgroup covers all rows of a
   * <= 96-row chunk; 16 / 32 = the row tiles are dealt to grid.z (more, lighter workgroups for GEMMs that run without
   * split-K).  wide_wg != 0: 16-wave workgroups where that keeps a long K to one pass (16 rows per workgroup only). */
  int rows_per_wg, wide_wg;
  /* ITTS_EPI_QKV_CACHE into a paged cache (see "Paged KV cache"): block table and block size, or NULL / 0 */
  const int32_t* kv_tab;
  int kv_bs;
  /* Packed-activation layout (see "Packed activation layout" above): x_packed -- x is packed [K/KS][ceil(M/16)][64][E];
   * y_packed -- y (ITTS_EPI_STORE / ITTS_EPI_GELU_STORE / ITTS_EPI_SILU_STORE / ITTS_EPI_RESID_F32, N % KS == 0) is written packed.
   * y_row0 / y_mtp (packed y only; 0 / 0 = the rows are the whole operand): the M rows land at rows [y_row0, y_row0 + M) of a
   * packed operand of y_mtp row tiles (y_row0 % 16 == 0) -- the Perceiver's [latents ; context] operand is written by two GEMMs.
   * x_mtp (packed x only; 0 = ceil(M / 16)): x is the first M rows of a packed operand of x_mtp row tiles. */
  int x_packed, y_packed;
  int y_row0, y_mtp, x_mtp;
  const float* post_scale; /* [N], ITTS_EPI_RELU_AFFINE_* only */
  const float* post_shift;
  const float* w_scale; /* [N]: itts_gemm_skinny_w8 only (wp holds packed E4M3 codes, see below); itts_gemm_skinny refuses a
                           non-NULL w_scale, so an FP8 image is never read as 16-bit weights */
} itts_skinny_args;
int itts_gemm_skinny(const itts_skinny_args* a, void* stream);
/* launch geometry itts_gemm_skinny would use: out8 = {grid.x, grid.y, waves per workgroup, column tiles per workgroup,
 * k-steps per wave, dynamic LDS bytes, grid.z, row tiles per workgroup} (host-only, launches nothing) */
int itts_skinny_plan(int dtype, int M, int N, int K, int ksplit, int rows_per_wg, int wide_wg, int fold, int* out8);

/* ------------------------------------------------------------------------------------------------------------------
 * FP8 (OCP E4M3, "e4m3fn") weight-only forms of the decode-step GEMM.
 *
 * Scheme.  A weight matrix W[K][N] is stored as one E4M3 code per element plus one fp32 scale per output column:
 *     W[k][n] ~ w_scale[n] * decode(code[k][n]),   w_scale[n] = max_k |W[k][n]| / 448   (indextts/utils/quant.py).
 * Codes are OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7f / 0xff are NaN and never produced by
 * the quantiser (the kernel does not treat them specially: they must not be fed).  Activations,
 * accumulation (fp32), the KV cache, the LayerNorm statistics and every epilogue stay as in the 16-bit kernel: a code is
 * converted IN REGISTERS to the activation type T (bf16 or f16; exact, every finite E4M3 value -- subnormals included -- is
 * representable in both) and feeds the same 16x16x32 MFMA as the A operand.
 *
 * Packed FP8 weight layout.  1-KiB blocks, each 16 columns x 64 k:
 *     block(nt, kb),  nt = n / 16 in [0, ceil(N / 16)),  kb = k / 64 in [0, ceil(K / 64)),  at byte ((nt * KB + kb) * 1024),
 *                     KB = ceil(K / 64); zero codes (0x00) pad K to a multiple of 64 and N to a multiple of 16.
 *     inside a block: lane l = (g << 4) | c (g = 0..3, c = 0..15) owns 16 contiguous bytes:
 *                     byte e     (e = 0..7) = code[kb * 64      + g * 8 + e][nt * 16 + c]
 *                     byte 8 + e (e = 0..7) = code[kb * 64 + 32 + g * 8 + e][nt * 16 + c]
 * i.e. the low 8 bytes are lane l's fragment of the 32-k step 2 kb and the high 8 bytes its fragment of step 2 kb + 1, in the k
 * order of the 16-bit packed weight layout and of the packed activation layout (lane (g, r) of k-step s holds k = 32 s + 8 g +
 * 0..7): one 16-byte load per lane yields the two complete 16x16x32 A fragments the 16-bit kernel loads as two blocks, and the
 * activations are read unchanged.
 * ------------------------------------------------------------------------------------------------------------------ */
/* bytes of the packed image: ceil(N / 16) * ceil(K / 64) * 1024 */
int64_t itts_packed_bytes_w8(int K, int N);
/* codes uint8 [K][N] row-major (device) -> packed (device), the layout above */
int itts_pack_weight_w8(const void* codes, void* packed, int K, int N, void* stream);

/* Y[M][N] = epi( w_scale[n] * (X[M][K] @ decode(codes)[K][N]) + bias ): itts_gemm_skinny over FP8 weights, with wp = the packed
 * E4M3 codes (itts_pack_weight_w8) and w_scale [N] (required).  Epilogue order: the accumulator is multiplied by w_scale[n] FIRST,
 * then everything the 16-bit epilogue does; LayerNorm folded (ln_c != NULL):
 *     v = rstd[m] * ( w_scale[n] * acc[m][n] - mean[m] * ln_c[n] ) + bias[n],   ln_c[n] = w_scale[n] * sum_k decode(code[k][n])
 * (the caller sums in float64), so a constant row cancels as in the 16-bit form.
 * dtype: ITTS_BF16 or ITTS_F16 (the activation type; ITTS_F32 is refused).  Epilogues: ITTS_EPI_STORE, _GELU_STORE, _RESID_F32,
 * _QKV_CACHE, _STORE_F32 (what the "fold" decode step and the head use); the split-K slab, _SILU_STORE and the
 * ITTS_EPI_RELU_AFFINE_* epilogues are refused (post_scale / post_shift are therefore never read), as is ksplit > 1.
 * wide_wg is the hint it is in itts_gemm_skinny: there is no 16-wave FP8 form, so it is ignored.
 * K % 32 == 0 (the activations' k-steps; the weight image is padded to 64).  Up to 96 rows per launch; more rows go 96 at a time
 * or, with rows_per_wg > 0, in one launch whose row tiles are dealt to grid.z. */
int itts_gemm_skinny_w8(const itts_skinny_args* a, void* stream);
/* launch geometry itts_gemm_skinny_w8 would use: out8 = {grid.x, grid.y, waves per workgroup, column tiles per workgroup,
 * 64-k weight blocks per wave, dynamic LDS bytes, grid.z, row tiles per workgroup} (host-only, launches nothing) */
int itts_skinny_plan_w8(int dtype, int M, int N, int K, int rows_per_wg, int fold, int* out8);

/* ------------------------------------------------------------------------------------------------------------------
 * FP8 (OCP E4M3, "e4m3fn") KV cache of the paged sampling loop.
 *
 * Format.  The paged pool ("Paged KV cache" above) holds one E4M3 code per cached element, uint8 [blocks][H][bs][64]
 * per layer, K and V separate, addressed through the same block table as the 16-bit pool.  One fp32 scale per (layer, K | V,
 * head): kv_scale float [2][H] of the layer a call works on (k scales, then v scales),
 *     k[j][d] ~ kv_scale[0][h] * decode(kcode[j][d]),     v[j][d] ~ kv_scale[1][h] * decode(vcode[j][d]).
 * Scales are positive powers of two: multiplying by the inverse is exact, so the device quantiser and the host quantiser
 * (indextts/utils/quant.py, quantize_kv_e4m3) give the same code for every input, and dequantisation commutes with every sum.
 * Quantiser: code = rne_e4m3( clamp(x / scale, -448, 448) ); the clamp is done in fp32 in front of the hardware conversion, so
 * nothing rests on a conversion's overflow rule.  0x7f / 0xff (NaN) are never produced.
 * ------------------------------------------------------------------------------------------------------------------ */
/* One decode step's attention of one layer over an FP8 paged cache, INCLUDING the append of the step's own key / value.
 *   qkv      T [B][3 * H * 64] row-major (the QKV GEMM's ITTS_EPI_STORE output): q | k | v of the step's token, per row.
 *   kcache / vcache  uint8 pools of this layer; kv_tab int32 [B][ITTS_KV_TAB]; kv_bs in {16, 32, 64}.
 *   kv_scale float [2][H].   pad int32 [B], pos int32 [1] (device): the row's keys are positions [pad[b], pos[0]) of the pool
 *   plus the new key, whose codes are stored at position pos[0] (64 + 64 bytes per (row, head), one owner per element: the
 *   workgroup of that (row, head)).  The new key takes part through its DECODED codes: the token sees what later tokens will see.
 *   skip_rows int32 [B] or NULL: a row with a nonzero entry neither appends nor writes its slice of `out`.
 *   out T: packed activation layout (out_packed != 0) or row-major [B][H * 64], as itts_attn_decode.
 * dtype: ITTS_BF16 or ITTS_F16 (ITTS_F32 is refused).  No beam row table, no shared-prefix reads, no contiguous cache. */
int itts_attn_decode_kv8(const void* qkv, void* kcache, void* vcache, void* out, const int32_t* pad, const int32_t* pos,
                         const float* kv_scale, int B, int H, int dtype, int out_packed, const int32_t* skip_rows,
                         const int32_t* kv_tab, int kv_bs, void* stream);

/* The prefill's keys / values of one layer into the FP8 pool: reads the k / v thirds of qkv T [rows][3 * H * 64], quantises with
 * the head's scales and scatters through the block table.  Two row addressings (those of itts_attn_prefill):
 *   row_off == NULL: rows [B][S]; local row s of element b goes to position s; rows in front of pad[b] (pad may be NULL) are
 *                    not stored.
 *   row_off != NULL: packed rows, element b owns rows [row_off[b], row_off[b + 1]) (at most S of them); local row s goes to
 *                    position cache_shift[b] + s (cache_shift may be NULL: 0).
 * 16 bytes of codes per thread. */
int itts_kv8_store(const void* qkv, void* kcache, void* vcache, const float* kv_scale, const int32_t* pad,
                   const int32_t* row_off, const int32_t* cache_shift, int B, int S, int H, int dtype, const int32_t* kv_tab,
                   int kv_bs, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Tiled MFMA GEMM / 1-D convolution, channels-last.
 *   acc(b,t,n) = sum_{j<taps} sum_{c<Cin} X[b][t + off0 + j*dil][c] * W[j][c][n]      (rows outside [0,Tin) are zero)
 *   v = scale * (act(acc + bias[n] + bias2[b][n]) + resid(b,t,n))
 *   y(b,t,n) = (accumulate ? y(b,t,n) : 0) + v
 * element (b,t,n) of y / resid lives at base + b*y_bstride + (t*N + n + y_shift), and is touched only when
 * 0 <= t*N + n + y_shift < y_limit.  A plain GEMM is taps=1, off0=0, B=1, Tin=Tout=M.  A transposed convolution with
 * stride u, kernel 2u (or u) is a 2-tap (1-tap) convolution with N = u*Cout and y_shift = -pad*Cout.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct itts_conv_args {
  int dtype;
  int B, Tin, Tout, Cin, N;
  int taps, off0, dil;
  const void* x;
  int64_t x_bstride; /* elements between batches of x */
  const void* wp;    /* packed [taps][ceil(N/16)][ceil(Cin/KS)] blocks */
  const float* bias; /* [N] or NULL */
  const float* bias2; /* [B][N] or NULL */
  int act;            /* 0 none, 1 gelu_new */
  void* y;
  int y_f32; /* y and resid are fp32 instead of T */
  int64_t y_bstride, y_shift, y_limit;
  const void* resid; /* same mapping as y, or NULL */
  int accumulate;
  float scale;
  /* ragged batches (NULL = every batch element has Tin valid rows): int32 [B] on the device; input rows >= valid_rows[b]
   * of batch element b read as zeros -- the convolution's own zero padding, so each element equals a run on its own --
   * and output tiles that only see that padding are not computed (their rows of y are left untouched). */
  const int32_t* valid_rows;
  /* split-K of a plain GEMM (taps = 1, B = 1, N % 128 == 0; 0 / 1 = off, <= 64): the K range is cut into ksplit slices that run as
   * separate tiles of ONE launch, and y (fp32, y_f32 = 1) receives the slabs [ksplit][Tout][N] -- slice ks holds the rows' partial
   * products over its K range: with KT = Cin / KS k-steps (KS = 32 columns, 16 at fp32; Cin % KS == 0, ksplit <= KT, Tin == Tout,
   * off0 = 0, no valid_rows) slice ks covers k-steps [(ks * KT) / ksplit, ((ks + 1) * KT) / ksplit), and y_bstride / y_shift /
   * y_limit are not read (slab ks starts at y + ks * Tout * N); no bias / bias2 / resid / accumulate / act (itts_ln_reduce sums the slabs in order, adds the bias
   * and the residual and applies the LayerNorm that follows; itts_rows sums any number of them).  For GEMMs with few output tiles (the prefill's N = 1280 projections:
   * 160 tiles of 128 x 128 for 512 workgroup slots). */
  int ksplit;
} itts_conv_args;
int itts_gemm_conv(const itts_conv_args* a, void* stream);


/* ------------------------------------------------------------------------------------------------------------------
 * Per-row LoRA adapter bank (many fine-tuned voices in one batch): the shrink half.
 *   y = x W + s_a (x A_a^T) B_a^T = [x | u] [W ; B_bank^T],   a = ids[m] the adapter of row m
 * The consuming GEMM (itts_gemm_skinny / itts_gemm_conv) runs unchanged with K' = K + Kx over a weight that was packed from
 * [W ; B_bank^T] (B_bank^T: every adapter's B^T, rp rows each, zero-padded); this launch writes the Kx extra operand columns:
 *   u[m][a * rp + j] = sum_k x[m][k] A_bank[a][j][k]   (j < rp; fp32 accumulation, one rounding to T, no atomics: deterministic)
 *   every other column of u[m][0 .. Kx) = 0;  a row with ids[m] < 0 (the base voice) is all zeros.
 * ALL Kx columns are written on every call (the buffers are reused across batches).
 *   x       T [M][K] row-major, or (x_packed) the packed activation layout with x_mtp row tiles (0 = ceil(M / 16))
 *   ids     int32 [M] on the device, read by the kernel: a captured graph serves any assignment of adapters to rows
 *   a_bank  T [n][rp][K]: adapter a's lora_A with its scaling alpha / r folded in (in fp32, before the rounding to T); rows past the
 *           adapter's own rank are zero.  rp = 16 * ceil(r_max / 16) <= 64;  Kx = n * rp rounded up to a multiple of 32, <= 512
 *   u       u_packed: the first block BEHIND the K / KS * u_mtp KiB of a packed operand [M][K] -- the operand's k-steps
 *           K / KS .. (K + Kx) / KS - 1 (u_mtp row tiles, 0 = ceil(M / 16); the tiles' padding rows are written as zeros);
 *           else row-major: element (m, j) at u + m * ldu + j (ldu in elements, a multiple of 16 bytes: u may point at column K
 *           of a [M][K + Kx] operand).
 * K % KS == 0; x, u and a_bank 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Per-row adapter BLENDS of the bank: the shrink half over weighted mixes of bank voices (itts_lora_shrink_mix).
 * The bank's identity holds for a weighted sum of adapters as it stands:
 *   y = x W + sum_j w_j s_{a_j} (x A_{a_j}^T) B_{a_j}^T = [x | u] [W ; B_bank^T]
 * with u non-zero in the slot of EVERY adapter the row names, each slot scaled by that entry's weight.  The consuming GEMMs, the
 * [W ; B_bank^T] weights and a_bank are those of itts_lora_shrink; only the launch that writes u differs. */
#define ITTS_LORA_MIX_ENTRIES 4

/* One row's mix: 32 bytes, 16-byte aligned.  Entry j = (id[j], weight[j]) is laid out as {int32 id; float weight} at byte 8 * j.
 *   id      adapter of the bank, in [0, n); -1 = empty entry.  Empty entries may stand anywhere; the ids of one record are
 *           distinct (the host enforces it; of two entries with one id the kernel writes the earlier).  An id outside the bank is
 *           treated as empty and reads nothing.
 *   weight  any finite fp32: not necessarily positive, no sum is prescribed.  1.0f = the adapter at the strength it was trained at.
 * A record with four empty entries is the base voice (u = 0). */
typedef struct __attribute__((aligned(16))) itts_lora_mix_row {
  struct {
    int32_t id;
    float weight;
  } e[ITTS_LORA_MIX_ENTRIES];
} itts_lora_mix_row;

/* One argument struct for both launches: itts_lora_shrink needs `ids` (and does not read `mix`), itts_lora_shrink_mix needs `mix`
 * (and does not read `ids`); every other field means the same to both (same layouts, limits and refusals). */
typedef struct itts_lora_shrink_args {
  int dtype;
  int M, K;
  const void* x;
  int x_packed, x_mtp;
  const int32_t* ids;
  const void* a_bank;
  int n, rp, Kx;
  void* u;
  int u_packed, u_mtp;
  int64_t ldu;
  const itts_lora_mix_row* mix; /* itts_lora_shrink_mix: [M] on the device, 16-byte aligned */
} itts_lora_shrink_args;
int itts_lora_shrink(const itts_lora_shrink_args* a, void* stream);

/* itts_lora_shrink over mixes: `mix` takes the part of `ids`.
 *   u[m][a_j * rp + r] = round_T( w_j * sum_k x[m][k] A_bank[a_j][r][k] )   for every non-empty entry j of mix[m]   (r < rp)
 *   every other column of u[m][0 .. Kx) = 0; the padding rows of a packed tail = 0.  ALL Kx columns are written on every call.
 * The sum is accumulated in fp32 in the order of itts_lora_shrink, the weight is applied in fp32, and the product is rounded to T
 * once: a record {a, 1.0f} gives the bits itts_lora_shrink gives for ids[m] = a.  No atomics; the order of a record's entries
 * does not change a bit of the result.
 *   mix     itts_lora_mix_row [M] on the device, read by the kernel: a captured graph serves any assignment of mixes to rows */
int itts_lora_shrink_mix(const itts_lora_shrink_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The JOIN of continuous batching: staged rows enter a running decode loop in one launch.
 *
 * Between two replays of the captured decode step, GPTEngine.decode_refill hands the slots of finished rows to new utterances
 * whose prompts were prefilled beside the loop (keys / values kept aside, first token sampled from their own logits).  This
 * launch moves all of it into the loop's buffers: the staged keys and values into the cache, and each entering row's state --
 * with the 32-byte voice record of its slot (itts_lora_mix_row) -- into the per-slot tables the captured step reads.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Keys / values.  For every staged position m in [0, M), layer l in [0, L) and head h in [0, H):
 *   kc[l * s_l + i_b[m] * s_b + h * s_h + i_p[m] * s_p + (0 .. 63)] = kst[((m * L + l) * H + h) * 64 + (0 .. 63)]    (vc <- vst alike)
 * The strides are in ELEMENTS, so one kernel serves the paged pool T [L][blocks][H][bs][64] (i_b = block, i_p = offset in the
 * block: s_l = blocks*H*bs*64, s_b = H*bs*64, s_h = bs*64, s_p = 64) and the contiguous cache T [L][rows][H][Smax][64] (i_b = cache
 * row, i_p = position).  Every stride is a multiple of 16 bytes' worth of elements and s_p >= 64 (checked); every 16-byte piece
 * has one owner, loaded and stored once.  A position with i_b[m] outside [0, n_b) or i_p[m] outside [0, n_p) is skipped
 * (memory guard; the host deals the positions), its neighbours are written.  The (i_b, i_p) pairs of one call are distinct.
 * dtype: ITTS_BF16 / ITTS_F16 (the serving types), or ITTS_F32 (the parity engine); the kernel moves bytes, no value is converted.
 *
 * Row state.  For every entering row j in [0, k) with slot s = rows[j] (skipped when s is outside [0, n_slots); the slots of one
 * call are distinct):
 *   tokens[s] = tok[j]     history[s * hist_cap] = tok[j]     finished[s] = fin[j]     force_stop[s] = stops[j]
 *   row_step0[s] = step0   pad[s] = pads[j]                   mix[s] = mix_new[j]      (mix / mix_new may both be NULL: no bank)
 * tok / fin are what the sample launch in front of this one (same stream) wrote for the new rows.
 * state[2] -= k (the entering slots were counted as finished): one thread, an ordinary read-modify-write -- nothing else touches
 * that word between two replays.
 * No allocation, no host synchronisation, no atomics; safe between graph replays on the loop's stream. */
typedef struct itts_refill_join_args {
  int dtype;
  int M, L, H;
  const void* kst; /* T [M][L][H][64] */
  const void* vst;
  void* kc;
  void* vc;
  int64_t s_l, s_b, s_h, s_p;
  int n_b, n_p;
  const int32_t* i_b; /* [M] */
  const int32_t* i_p; /* [M] */
  int k;
  int n_slots;
  const int32_t* rows; /* [k] */
  const int32_t* tok;  /* [k] */
  const int32_t* fin;
  const int32_t* stops;
  const int32_t* pads;
  const itts_lora_mix_row* mix_new; /* [k] or NULL */
  int step0;
  int hist_cap;
  int32_t* tokens; /* [n_slots] each */
  int32_t* history; /* [n_slots][hist_cap] */
  int32_t* finished;
  int32_t* force_stop;
  int32_t* row_step0;
  int32_t* pad;
  itts_lora_mix_row* mix; /* [n_slots] or NULL */
  int32_t* state;         /* the loop's state words; [2] = finished rows */
} itts_refill_join_args;
int itts_refill_join(const itts_refill_join_args* a, void* stream);

/* LayerNorm over the last dim of fp32 rows; y is T (y_f32 = 0) or fp32 (y_f32 = 1).  If w2 != NULL a second LayerNorm
 * (w2,b2) is applied to the result of the first (ln_f followed by final_norm). */
int itts_layernorm(const float* h, const float* w, const float* b, const float* w2, const float* b2, void* y, int y_f32,
                   int M, int D, int dtype, void* stream);

/* Residual update + LayerNorm for the decode step:
 *   if (nslab > 0)  h[m][:] += bias[:] + slab[0][m][:] + ... + slab[nslab-1][m][:]      (fixed order; h updated in place)
 *                   [+ runtime LoRA, below]
 *   y[m][:] = LN(h[m][:]; w, b)   (then LN(.; w2, b2) if w2 != NULL),  y is T [M][D].
 * nslab <= 6.  slab is fp32 [nslab][M][slab_stride] as written by itts_gemm_skinny(ITTS_EPI_SLAB_F32) with N = slab_stride (0 = D).
 * y_packed != 0 (needs D % 256 == 0): y is written in the packed activation layout.
 * state_bump (int32[2] device words or NULL): both words are incremented once by this launch -- the decode loop's step
 * counter and cache position, advanced here (a launch that reads neither) instead of by the sampling kernel.
 * Runtime LoRA of the producing projection (lora_b != NULL; unmerged adapters, peft convention y = x W + (x A^T) B^T alpha/r):
 * the projection's packed weight carries A^T * alpha/r as lora_r extra output COLUMNS (N = D + 16*ceil(r/16) in the
 * GEMM), so slab columns [D, D + r) hold the split-K partials of x A; this kernel adds (sum of those) @ lora_b, with lora_b
 * = B^T fp32 [r][D].  The LoRA A.B product is thereby fused into the output projection + its residual update: no extra
 * launch, no merged copy of the weight. */
typedef struct itts_ln_reduce_args {
  int dtype, M, D;
  float* h;
  const float* slab;
  int nslab, slab_stride;
  const float* bias;
  const float* w;
  const float* b;
  const float* w2;
  const float* b2;
  void* y;
  int y_packed;
  int32_t* state_bump;
  const float* lora_b;
  int lora_r;
} itts_ln_reduce_args;
int itts_ln_reduce(const itts_ln_reduce_args* a, void* stream);

/* h[b][:] = table[tokens[b]][:] + pos_table[p][:],  p = clamp(*step - row_step0[b] + pos_add, 0, pos_rows - 1)
 * (fp32 tables, fp32 h; pos_rows = rows of pos_table: a finished slot that keeps stepping never reads past the table).
 * bump (device word or NULL) is incremented once by the launch: the decode loop's cache position, which this launch does
 * not read.  h_packed (T, packed activation layout for M = B rows, or NULL): a T-typed copy of the same rows -- the operand
 * of the first LayerNorm-folded GEMM of the step.
 * row_step0 (int32 [B] on the device or NULL = zeros): the loop step at which row b started decoding -- a decode slot that
 * was refilled with a new utterance in the middle of the loop counts its mel positions from its own first token. */
int itts_embed_step(const int32_t* tokens, const float* table, const float* pos_table, const int32_t* step, int pos_add,
                    float* h, int B, int D, int32_t* bump, const int32_t* row_step0, int pos_rows, void* h_packed, int dtype,
                    void* stream);

/* Single-query attention over the KV cache (decode).  q,out: T [B][H*64]; caches T [B][H][smax][64];
 * keys j in [pad[b], *pos] are visible (the key at *pos was just appended).  scale 1/8.  out_packed != 0: out is written in
 * the packed activation layout (M = B, K = H*64).
 * kv_rows / kv_step (both or neither): beam search without cache copies -- position j of logical row b is read from
 * physical cache row kv_rows[(*kv_step & 1)][b][j] (int32 [2][B][smax], maintained by itts_beam_kv_rows).
 * Entries of different rows may name the SAME physical row (the beams of a batch element share their prompt and common
 * history; the engine caches the prompt once per batch element).
 * skip_rows (int32 [B] on the device or NULL): rows with a nonzero entry are left out (out[b] keeps its old contents) --
 * the decode loop passes its `finished` flags, a finished row's logits no longer matter.
 * kv_share (one int32 word on the device, or NULL): (p0 << 8) | C with C <= 255 -- a promise that the first C keys / values of
 * every row, positions [pad[b], pad[b] + C), hold the same bytes as cache row 0's positions [p0, p0 + C) (a one-prompt
 * batch's conditioning latents after itts_attn_prefill_shared); they are then read from row 0 (one L2-resident copy instead
 * of B copies from HBM).  0 = no sharing.  Ignored with kv_rows. */
int itts_attn_decode(const void* q, const void* kcache, const void* vcache, void* out, const int32_t* pad,
                     const int32_t* pos, int B, int H, int smax, int dtype, int out_packed, const int32_t* kv_rows,
                     const int32_t* kv_step, const int32_t* skip_rows, const int32_t* kv_share, const int32_t* kv_tab, int kv_bs,
                     void* stream);

/* Causal self-attention over a whole (left-padded) sequence.  qkv: T [B][S][3*H*64] (q|k|v); out: T [B][S][H*64];
 * query i sees key j iff pad[b] <= j <= i; rows with no visible key produce zeros.  If kcache/vcache are non-NULL the
 * k/v rows are also written to the caches (T [B][H][smax][64]) at rows [0,S). */
int itts_attn_prefill(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* pad, int B, int S, int H,
                      int smax, int dtype, void* stream);

/* The same over PACKED rows: no padding rows exist; the rows of batch element b are [row_off[b], row_off[b+1]) of qkv /
 * out (row_off: int32 [B+1], device), each at most Smax long, plain causal attention inside each element.  With caches,
 * local row i of element b is written to cache row cache_shift[b] + i (cache_shift NULL = 0): with cache_shift = the
 * element's left padding this reproduces the cache layout of the padded form. */
int itts_attn_prefill_packed(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* row_off,
                             const int32_t* cache_shift, int B, int Smax, int H, int smax, int dtype, const int32_t* kv_tab,
                             int kv_bs, void* stream);

/* Packed rows behind a CACHED PREFIX (the teacher-forced latent pass, model.py:459-474 / 548-597, for a batch whose prompt the
 * decode loop has cached): element b's sequence is  pre_len[b] keys / values read from cache row pre_row[b], positions
 * pre_pos0[b] .. pre_pos0[b] + pre_len[b] - 1 (caches T [rows][H][smax][64], read only)  |  its rows [row_off[b], row_off[b+1])
 * of qkv.  Only the qkv rows are queries (query i sits at sequence position pre_len[b] + i and sees every key up to it); out has
 * the rows of qkv.  Key tiles are cut from sequence position 0, so every output row equals, bit for bit, the row
 * itts_attn_prefill_packed produces when the prefix's k / v rows are part of qkv. */
int itts_attn_prefill_prefix(const void* qkv, void* out, const void* kcache, const void* vcache, const int32_t* row_off,
                             const int32_t* pre_len, const int32_t* pre_row, const int32_t* pre_pos0, int B, int Smax, int H,
                             int smax, int dtype, const int32_t* kv_tab, int kv_bs, void* stream);

/* Packed rows behind a prefix that is SHARED and computed in the same pass (the prefill of a batch whose elements all start
 * with the same conditioning latents, model.py:606-667 with one prompt: those rows see only themselves, so their hidden states
 * are the same in every element and are computed once).  Element e of the E packed elements owns rows [row_off[e],
 * row_off[e+1]) of qkv / out; its sequence is  pre_len[e] keys taken from qkv rows pre_row0[e] .. pre_row0[e] + pre_len[e] - 1
 * (k / v thirds of those rows)  |  its own rows.  pre_len[e] = 0 for the shared block itself.  Same key tiling from sequence
 * position 0 as itts_attn_prefill_packed over the un-shared layout: same bits per row.  With caches (T [rows][H][smax][64]),
 * element e's OWN rows are appended to cache row w_row[e] at positions w_pos0[e] + local row (the caller copies the shared
 * block's cache rows to the other elements' cache rows).
 *
 * pre_row0 == NULL selects the CACHED-PREFIX APPEND form (the incremental latent pass of a stream, which keeps the keys and
 * values of every row it has computed): element e's sequence is  pre_len[e] keys / values read from cache row w_row[e],
 * positions [w_pos0[e] - pre_len[e], w_pos0[e])  |  its own rows [row_off[e], row_off[e+1]) of qkv.  Only the qkv rows are
 * queries (query i sits at sequence position pre_len[e] + i and sees every key up to itself), and the k / v thirds of the own
 * rows are appended to cache row w_row[e] at positions w_pos0[e] + i.  The caches are required (kcache, vcache, w_row, w_pos0
 * non-NULL) and contiguous, T [rows][H][smax][64]; kv_tab != NULL is refused.  What a launch reads from the caches (< w_pos0[e])
 * and what it writes (>= w_pos0[e]) never overlap; the keys of the new rows are taken from qkv, never read back.  The caller
 * guarantees 0 <= w_pos0[e] - pre_len[e], w_pos0[e] + rows of e <= smax and distinct w_row (device data: not checked).
 * Key tiles are cut from sequence position 0 in steps of 64 and one query row's arithmetic is that of the other forms, so every
 * output row equals, bit for bit, the row itts_attn_prefill_packed produces for the same sequence with the prefix rows inside
 * qkv.  Two kernel forms, chosen from Smax, with the same bits per row: Smax <= 128 runs a 16-query tile per workgroup
 * (itts_last_kernel() = "attn_append<16>"), anything longer the 64-query tile of the other forms ("attn_append<64>"); Smax may
 * exceed the longest element (workgroups past an element's rows return at once). */
int itts_attn_prefill_shared(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* row_off,
                             const int32_t* pre_len, const int32_t* pre_row0, const int32_t* w_row, const int32_t* w_pos0,
                             int E, int Smax, int H, int smax, int dtype, const int32_t* kv_tab, int kv_bs, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Token selection for one decode step, on device (no host sync in the loop).
 * state (int32[8], device): [0] = step k (number of tokens already generated), [1] = cache position of the NEXT token
 * to be fed, [2] = number of finished rows.  The kernel reads logits (fp32 [B][V]), applies repetition penalty over
 * {extra_ids} U history[b][0..k), temperature, top-k, top-p, draws (Philox4x32-10 keyed by seed, counter (row,k,0,0))
 * or takes the argmax, then appends to history, updates tokens/finished, and increments state[0], state[1].
 * Rows already finished, or with force_stop[b] == k, emit stop_token.
 * Capacity: a row keeps at most 1024 candidates.  If more than 1024 scores are at or above the k-th value (ties with it are kept),
 * the 1024 that stay are whichever reach the candidate store first: the token is one of the tied set, but not reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */
/* itts_sample_rows: the step with PER-ROW sampling settings.  A device table of one record per row replaces the scalar parameters, so a
 * row of a batch -- or a slot of a refilled loop -- keeps its own request's settings and one captured launch serves every
 * assignment (the records are data, like the adapter ids of itts_lora_shrink).  Row b is processed exactly as itts_sample
 * processes a row under the scalars of rows[b]; greedy and sampling rows may share a launch.
 * Record: 32 bytes, 16-byte aligned (a workgroup fetches its row's record as two 16-byte words):
 *   byte  0  float    rep_penalty
 *         4  float    temperature
 *         8  float    top_p
 *        12  int32    top_k
 *        16  uint64   seed       Philox key = seed + the 64-bit value in state[4..5]
 *        24  uint32   stream     Philox counter = (stream, k_b, 0, 0) with the row's OWN step k_b = state[0] - row_step0[b]:
 *                                what a request draws depends on its seed, stream and step, not on its slot or on when it
 *                                entered.  stream = b without row_step0 is itts_sample's counter.
 *        28  int32    do_sample  0 = argmax (temperature, top_k, top_p unused)
 * The library cannot see the records at launch time.  The caller validates them before the upload (sampling rows: 1 <= top_k
 * <= 1024, 0 < top_p <= 1, temperature > 0; every row: rep_penalty > 0); the kernel itself only stays memory-safe for any
 * record: a sampling row's top_k is clamped into [1, min(V, 1024)], a temperature or penalty that is not > 0 is taken as 1,
 * the emitted token is clamped into [0, V).  The arguments are itts_sample_args with `rows` set; the scalar settings
 * (rep_penalty, temperature, top_p, top_k, do_sample, seed) are ignored. */
typedef struct itts_sample_row {
  float rep_penalty, temperature, top_p;
  int32_t top_k;
  uint64_t seed;
  uint32_t stream;
  int32_t do_sample;
} itts_sample_row;
typedef struct itts_sample_args {
  const float* logits;
  int B, V, ldl; /* ldl = row stride of logits */
  int32_t* tokens;   /* [B] out: token selected this step */
  int32_t* history;  /* [B][hist_cap] generated tokens */
  int hist_cap;
  int32_t* finished; /* [B] */
  int32_t* state;    /* [8] */
  const int32_t* extra_ids; /* ids always penalised (the fake prefix: 1 and 8192) */
  int n_extra;
  const int32_t* force_stop; /* [B] or NULL */
  float rep_penalty, temperature, top_p;
  int top_k, do_sample; /* do_sample != 0 requires 1 <= top_k <= 1024 (candidate store; top_k <= 0 is refused, not truncated) */
  uint64_t seed;     /* Philox key = seed + the 64-bit value in state[4..5] (lo, hi): a captured launch serves any seed */
  int stop_token;
  float* dbg_scores; /* optional [B][V] processed scores (-inf = removed), for parity tests; NULL in production */
  int no_advance;    /* != 0: leave state[0] / state[1] alone -- the caller advances them in the next step's first
                        itts_ln_reduce launch (state_bump), which removes a device-wide fence and a returning atomic
                        per row from this kernel; itts_embed_step is then given pos_add + 1 */
  const int32_t* row_step0; /* [B] or NULL (= zeros): loop step at which row b started (slot refill).  Row b's own step
                        k_b = state[0] - row_step0[b] indexes its history, bounds its repetition-penalty window and is what
                        force_stop[b] is compared with; the Philox counter stays (b, state[0]). */
  const itts_sample_row* rows; /* itts_sample_rows: [B] on the device, 16-byte aligned; itts_sample refuses a non-NULL rows */
} itts_sample_args;
int itts_sample(const itts_sample_args* a, void* stream);

/* itts_sample with the per-row settings of `rows` (the record and its rules: above, in front of itts_sample_args) */
int itts_sample_rows(const itts_sample_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Beam search / beam-sample step (num_beams > 1) -- replaces, for the generate() call at indextts/gpt/model.py:710-715,
 * transformers 4.44.2 GenerationMixin._beam_search + BeamSearchScorer.process + BeamHypotheses.add/is_done
 * (third-party; restated in oracle/beam_ref.py).  Rows are laid out batch-major: row = b*num_beams + beam.
 * One call = one decoding step for all batch elements: log-softmax, repetition penalty, (temperature, top-k, top-p with
 * min_tokens_to_keep = 2 when do_sample), running beam scores, 2*num_beams candidates drawn without replacement (own
 * Philox stream: counter (b, step, draw, 0)) or taken, scorer bookkeeping, hypothesis store, per-row token histories.
 * state[0] = step, state[1] = cache position (both advanced by the call), state[2] = finished batch elements.
 * Capacity: a batch element's pool is its beams' sorted candidate lists concatenated in beam order and cut at 1024 entries BEFORE
 * it is sorted, so when ties at a row's k-th score make the lists longer than 1024 in all, the last beams lose their lowest candidates.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct itts_beam_args {
  const float* logits; /* [B*num_beams][ldl] */
  int B, num_beams, V, ldl;
  int32_t* tokens;      /* [B*num_beams] out: token appended to each row */
  int32_t* src;         /* [B*num_beams] out: row (absolute index) each row continues */
  float* beam_scores;   /* [B*num_beams] in/out: running sum of log-probabilities (init 0, -1e9, -1e9, ... per batch element) */
  int32_t* hist;        /* [2][B*num_beams][hist_cap] generated tokens, ping-pong by step parity (input = step & 1) */
  int hist_cap;
  float* hyp_score;     /* [B][num_beams] closed hypotheses: score, generated length, tokens */
  int32_t* hyp_len;
  int32_t* hyp_tok;     /* [B][num_beams][hist_cap] */
  int32_t* n_hyp;       /* [B] */
  float* worst;         /* [B] lowest score among the closed hypotheses (init +1e9) */
  int32_t* done;        /* [B] */
  int32_t* state;       /* [8] */
  const int32_t* extra_ids; /* ids always penalised (the fake prefix: 1 and 8192) */
  int n_extra;
  float rep_penalty, temperature, top_p, length_penalty;
  int top_k, do_sample; /* do_sample != 0 requires 1 <= top_k <= 128 (one 1024-entry candidate pool per batch element) */
  uint64_t seed;        /* Philox key = seed + the 64-bit value in state[4..5], as in itts_sample_args */
  int eos_token;
  /* scratch between the step's two launches (per-row candidates -> per-batch-element pooling); caller-owned, no init:
   * cand_scores / cand_ids [B*num_beams][ITTS_BEAM_CAND] each, cand_n [B*num_beams] */
  float* cand_scores;
  int32_t* cand_ids;
  int32_t* cand_n;
} itts_beam_args;
#define ITTS_BEAM_CAND 1024
int itts_beam_step(const itts_beam_args* a, void* stream);

/* KV rows follow their beams as a TABLE (GPT2InferenceModel._reorder_cache, model.py:207-218, without moving cache bytes):
 * kv_rows int32 [2][rows][smax], ping-pong by step parity; entry [r][j] = physical cache row that holds position j of
 * logical row r (rows = B*num_beams).  Call right after itts_beam_step (state[0] = k+1, state[1] = P): table (k+1)&1 is
 * written from table k&1 -- [r][j] = old[src[r]][j] for j < P, and [r][P] = r (where the next step appends).  Start from
 * table 0 = identity.  itts_attn_decode reads the table through its kv_rows / kv_step arguments. */
int itts_beam_kv_rows(int32_t* kv_rows, const int32_t* src, const int32_t* state, int rows, int smax, void* stream);

/* The same by COPYING cache rows (kept as the reference form; the decode loop uses the table):
 * KV cache rows follow their beams (GPT2InferenceModel._reorder_cache, model.py:207-218): row r <- row src[r] for cache
 * positions [0, state[1]), every layer, K and V; batch elements whose rows map to themselves are skipped.
 * Cache layout [layers][rows][heads][smax][64]; layer_stride in elements. */
int itts_beam_reorder_kv(void* kcache, void* vcache, const int32_t* src, const int32_t* state, int layers, int B, int num_beams,
                         int heads, int smax, int64_t layer_stride, int dtype, void* stream);

/* Keys / values of cache positions [p0, p0 + C) of row 0 -> positions [pad[b], pad[b] + C) of rows 1 .. B-1, all `layers` layers in
 * one launch (layer l of a cache at + l * layer_stride elements): a one-prompt batch's conditioning rows, computed once by the
 * shared-prefix prefill (itts_attn_prefill_shared), reach every row's cache.  Both cache forms (kv_tab NULL = contiguous). */
int itts_kv_share_rows(void* kcache, void* vcache, int layers, int64_t layer_stride, int B, int H, int C, int p0, const int32_t* pad,
                       int smax, const int32_t* kv_tab, int kv_bs, int dtype, void* stream);

/* pcm[b][i] = trunc( clamp(32767 * tanh(x[b][i]), -32767, 32767) ) as int16; also writes fp32 wav if wav != NULL.
 * apply_tanh = 0 skips the tanh (input already in (-1,1)). */
int itts_tanh_pcm(const void* x, float* wav, int16_t* pcm, int64_t n, int dtype, int apply_tanh, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Prompt front-end: the Conformer + Perceiver conditioner of UnifiedVoice.get_conditioning (indextts/gpt/model.py:487-546;
 * conformer_encoder.py:167-290,360-386, conformer/subsampling.py:111-143, conformer/attention.py, perceiver.py:181-312) as a
 * chain of these launches and LayerNorm-folded itts_gemm_skinny calls over one prompt (~150 rows): bf16 / f16 only, fp32
 * residual stream, every GEMM operand in the packed activation layout.  The host side is indextts/gpt/conditioner.py.
 * ------------------------------------------------------------------------------------------------------------------ */
/* y (T [T2][C * F2], T2 = (T-3)/2+1, F2 = (F-3)/2+1) = relu(Conv2d(1, C, 3, stride 2)(mel [T][F])) laid out as the operand of
 * the Linear(C * F2 -> d) that follows: element (t, c * F2 + f).  w [C][9], b [C] fp32.  Exactly the T2 * C * F2 elements of y are
 * written. */
int itts_subsample_conv(const float* mel, const float* w, const float* b, void* y, int T, int F, int C, int dtype, void* stream);

/* Multi-head attention over a short sequence, head dim 64:  out[i] = softmax_j( scale * ((q_i + u) . k_j + (q_i + v) . p_j) ) v_j
 * for i < Tq, j < Tk.  q / k / v: T rows with the given strides (elements, multiples of 8), head h at columns [64 h, 64 h + 64).
 * pos (T [H][Tk][64], the layer's projected position table) with bias_u / bias_v (fp32 [H * 64]) = the Conformer's relative-
 * position attention WITHOUT rel_shift; pos = NULL: plain attention (the term and the biases are absent).  out: T in the packed
 * activation layout of a [Tq][H * 64] operand with out_mtp row tiles; rows >= Tq of the tiles are not written. */
typedef struct itts_mha_args {
  int dtype;
  int Tq, Tk, H;
  const void* q;
  const void* k;
  const void* v;
  int64_t q_stride, k_stride, v_stride;
  const void* pos;
  const float* bias_u;
  const float* bias_v;
  float scale;
  void* out;
  int out_mtp;
} itts_mha_args;
int itts_mha_small(const itts_mha_args* a, void* stream);

/* The Conformer convolution module between its pointwise convolutions: x (T [T][2 C], value | gate) -> GLU -> depthwise
 * Conv1d(taps, zero "same" padding; w fp32 [C][taps], b [C]) -> LayerNorm(ln_w, ln_b, eps) -> SiLU -> y (T, packed layout of
 * [T][C] with y_mtp row tiles; rows >= T of the tiles are not written).  C % 128 == 0, C <= 2048; taps 7 / 15 / 31. */
int itts_glu_dwconv_ln_silu(const void* x, const float* w, const float* b, const float* ln_w, const float* ln_b, void* y, int T,
                            int C, int taps, int y_mtp, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The prompt front-end over N prompts of different lengths in one launch each.
 *
 * The row-wise launches of the conditioner (the GEMMs, itts_rows, itts_geglu) run unchanged over the concatenated rows of all
 * prompts.  The three launches that mix rows of a sequence -- the subsampling convolution, the attention and the convolution
 * module -- exist here in a segmented form: the same kernel bodies as itts_subsample_conv, itts_mha_small and
 * itts_glu_dwconv_ln_silu behind a segment lookup, and a segment's result has the bits the single-prompt entry point gives for
 * that segment alone.
 *
 * Row space.  Segment s owns rows [row0, row0 + len) of the launch's row space, row0 a multiple of 16: a 16-row tile of a packed
 * operand never holds rows of two segments.  The rows between a segment's end and the next multiple of 16 are padding rows:
 * row-wise launches may compute on them, no entry point here reads them as data or writes them.
 *
 * Segment table.  int32 words: nseg records of ITTS_SEG_WORDS words, then `ntiles` words that name the segment of every 16-row
 * tile of the row space (-1: none).  It exists twice: `dev` in device memory is what the kernels read -- device DATA, so a captured
 * graph depends on the geometry (nseg, ntiles, and through the caller's buffers the lengths), never on the pointer's contents
 * being known at capture time -- and `host`, the same words in host memory, which the entry point checks (row0 % 16, len > 0,
 * no tile in two segments, every range inside its buffer) before it launches: an invalid table returns ITTS_ERR_INVALID and
 * launches nothing.  The caller keeps the two copies equal.
 *
 *   word  itts_subsample_conv_seg        itts_mha_small_seg                       itts_glu_dwconv_ln_silu_seg
 *   0     row0: first output row         row0: first query row                    row0: first row of x and y
 *   1     len = (T_p - 3) / 2 + 1        len: queries                             len: rows
 *   2     first frame of the prompt      first row of the first key range         -
 *   3     T_p: frames of the prompt      rows of the first key range (> 0)        -
 *   4     -                              first row of the second key range        -
 *   5     -                              rows of the second key range (0: none)   -
 *   6     -                              first output row (a multiple of 16)      -
 *   7     reserved (0)
 * ------------------------------------------------------------------------------------------------------------------ */
#define ITTS_SEG_WORDS 8

typedef struct itts_seg_table {
  const int32_t* dev;  /* device: nseg * ITTS_SEG_WORDS + ntiles words */
  const int32_t* host; /* the same words in host memory */
  int nseg, ntiles;
} itts_seg_table;

/* itts_subsample_conv over N prompts: mel fp32 [frames][F] holds the prompts' frames one after another (segment s: frames
 * [word 2, word 2 + word 3)), a 3 x 3 stride-2 window never leaves its prompt; y T [ntiles * 16][C * F2], row row0 + t of a
 * segment = what itts_subsample_conv writes to row t for that prompt alone.  Rows of y outside every segment are not written. */
int itts_subsample_conv_seg(const float* mel, const float* w, const float* b, void* y, const itts_seg_table* tab, int frames, int F,
                            int C, int dtype, void* stream);

/* itts_mha_small over N segments, one (segment, head, 16-query tile) per workgroup.  The fields of `a` keep their meaning with
 * these differences: q / k / v point at row 0 of their row spaces, a->Tq = rows of q and a->Tk = rows of k and v that exist
 * (bounds of the table); a segment's queries are rows [row0, row0 + len) of q, its keys and values the rows of its first key
 * range followed by those of its second; pos is T [H][pos_tk][64] and, like bias_u / bias_v, indexed by the key's index WITHIN
 * its segment (pos_tk >= the longest segment's key count; the first Tk rows of every head are those of the single-prompt table
 * for Tk keys); the output of query i of a segment goes to row (word 6) + i of the packed out operand of a->out_mtp row tiles.
 * Output rows outside every segment are not written; the caller keeps the segments' output rows apart. */
int itts_mha_small_seg(const itts_mha_args* a, const itts_seg_table* tab, int pos_tk, void* stream);

/* itts_glu_dwconv_ln_silu over N segments of x T [ntiles * 16][2 C] -> packed y of y_mtp >= ntiles row tiles: the depthwise
 * taps see zeros beyond the segment's first and last row, never the neighbouring segment's rows.  Rows outside every segment
 * are neither read nor written. */
int itts_glu_dwconv_ln_silu_seg(const void* x, const float* w, const float* b, const float* ln_w, const float* ln_b, void* y,
                                const itts_seg_table* tab, int C, int taps, int y_mtp, float eps, int dtype, void* stream);


/* Row operations on an fp32 residual stream [M][D] (D % 4 == 0, D <= 2048):
 *   v = (x ? x[m] : 0) + (bias ? bias : 0) + slab[0][m] + ... + slab[nslab-1][m]       (fixed order; slab fp32 [nslab][M][D])
 *   norm 1: v = LayerNorm(v; w, b, eps)     norm 2: v = v / max(|v|_2, 1e-12) * sqrt(D) * w     norm 0: as is
 *   y (fp32 [M][D], may alias x, or NULL) = v;   y_packed (T, or NULL): rows [y_row0, y_row0 + M) of a packed operand of y_mtp
 *   row tiles (0 = ceil(M / 16)); no other row of that operand is written.  */
typedef struct itts_rows_args {
  int dtype, M, D;
  const float* x;
  const float* slab;
  int nslab;
  const float* bias;
  int norm;
  const float* w;
  const float* b;
  float eps;
  float* y;
  void* y_packed;
  int y_row0, y_mtp;
} itts_rows_args;
int itts_rows(const itts_rows_args* a, void* stream);

/* y (T, packed layout of [M][Kp], y_mtp row tiles, 0 = ceil(M / 16)) = gelu(h[:, Kp:]) * h[:, :Kp]  (erf gelu; h T [M][2 Kp]).
 * Rows >= M of the tiles are not written. */
int itts_geglu(const void* h, void* y, int M, int Kp, int y_mtp, int dtype, void* stream);

/* The GPT prompt rows of UnifiedVoice.prepare_gpt_inputs (indextts/gpt/model.py:606-667): per batch row b the ids of text [B][L]
 * (int64) that are neither start_tok nor stop_tok (n of them, order kept) become start | ids | stop, embedded as
 * text_emb[id] + text_pos[j] (fp32 tables of n_tok / n_pos rows, j = index in that sequence), placed behind the C conditioning latents
 * (conds fp32 [conds_rows][C][D], conds_rows 1 = shared by all rows) and right-aligned in P = C + L + 2 positions:
 *   emb (fp32 [B][P][D]): L - n zero rows, the latents, the n + 2 text rows;  mask (int64 [B][P + 1]): 0 on the zero rows, else 1
 *   (the last slot is the start-mel token's);  pad (int32 [B]) = L - n.   L <= 2046, D % 4 == 0. */
int itts_prefix_rows(const int64_t* text, const float* conds, int conds_rows, const float* text_emb, const float* text_pos, float* emb,
                     int64_t* mask, int32_t* pad, int B, int L, int C, int D, int start_tok, int stop_tok, int n_tok, int n_pos,
                     void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Speaker encoder (ECAPA-TDNN, indextts/BigVGAN/ECAPA_TDNN.py:470-581) over one prompt: its 1 x 1 convolutions are
 * itts_gemm_skinny calls with the ITTS_EPI_RELU_AFFINE_* epilogues; the rest is below.  Activations are T-typed packed operands
 * [frames][channels] of `mtp` row tiles; bf16 / f16 only.  The host side is indextts/BigVGAN/speaker_engine.py.
 * ------------------------------------------------------------------------------------------------------------------ */
/* y (packed [T][Kp]) column j * F + f = x[reflect(t + (j - (taps-1)/2) * dil)][f] (x fp32 [T][F]), zeros from taps * F on: a k-tap
 * convolution with reflect "same" padding (nnet/CNN.py:430-488) becomes a plain GEMM over this operand.  Rows >= T of the y_mtp
 * tiles are not written. */
int itts_im2col_reflect(const float* x, void* y, int T, int F, int taps, int dil, int Kp, int y_mtp, int dtype, void* stream);
/* One step of a Res2Net block (scale 8, 64-channel chunks): cat[:, 64 c : 64 c + 64] = BN(relu(conv_k3_dil(y1 chunk c [+ cat chunk
 * c - 1 unless first]) + bias)), reflect padding; first also copies chunk 0 (cat[:, :64] = y1[:, :64]).  wp = itts_pack_weight of the
 * [3 * 64][64] matrix (row = tap * 64 + input channel); bias / scale / shift fp32 [64].  Rows >= T of y1 and cat (the padding rows of
 * the last tile) are neither read nor written, and no other column of cat is touched. */
int itts_res2_step(const void* y1, void* cat, const void* wp, const float* bias, const float* scale, const float* shift, int T, int mtp,
                   int chunk, int dil, int first, int dtype, void* stream);
/* gate (fp32 [C]) = sigmoid(w2 relu(w1 mean_t(y) + b1) + b2): the squeeze-and-excitation gate; w1 T [H][C], w2 T [C][H] row-major.
 * The mean runs over rows < T: the padding rows of y may hold anything. */
int itts_se_gate(const void* y, const void* w1, const float* b1, const void* w2, const float* b2, float* gate, int T, int C, int H,
                 int mtp, int dtype, void* stream);
/* out = gate[c] * y + res over packed [T][C] operands of one geometry (out may be a k-step run of a wider operand).  Whole row tiles
 * are mapped: the padding rows of out are written too, from the padding rows of y and res. */
int itts_scale_resid(const void* y, const void* res, const float* gate, void* out, int T, int C, int mtp, int dtype, void* stream);
/* Per-channel statistics over time of packed x [T][C]: weights w_t = softmax_t(logit[t][c]) (logit T row-major [T][C]) or 1 / T
 * (logit NULL); m = sum w x, s = sqrt(max(sum w (x - m)^2, 1e-12)); out (T [2 C]) = [m | s] * scale + shift (fp32 [2 C], or NULL):
 * the global-context statistics and the attentive statistics pooling + BatchNorm (ECAPA_TDNN.py:543-581).  The sums run over
 * rows < T: the padding rows of x may hold anything. */
int itts_col_stats(const void* x, const void* logit, const float* scale, const float* shift, void* out, int T, int C, int mtp, int dtype,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INDEXTTS_HIP_H */
