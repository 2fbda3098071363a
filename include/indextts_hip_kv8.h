/*
 * indextts_hip_kv8.h -- FP8 (OCP E4M3, "e4m3fn") KV cache of the paged sampling loop.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  The Python side lists these entry points as _native.KV8_SYMBOLS.
 *
 * Format.  The paged pool (indextts_hip.h, "Paged KV cache") holds one E4M3 code per cached element, uint8 [blocks][H][bs][64]
 * per layer, K and V separate, addressed through the same block table as the 16-bit pool.  One fp32 scale per (layer, K | V,
 * head): kv_scale float [2][H] of the layer a call works on (k scales, then v scales),
 *     k[j][d] ~ kv_scale[0][h] * decode(kcode[j][d]),     v[j][d] ~ kv_scale[1][h] * decode(vcode[j][d]).
 * Scales are positive powers of two: multiplying by the inverse is exact, so the device quantiser and the host quantiser
 * (indextts/utils/quant.py, quantize_kv_e4m3) give the same code for every input, and dequantisation commutes with every sum.
 * Quantiser: code = rne_e4m3( clamp(x / scale, -448, 448) ); the clamp is done in fp32 in front of the hardware conversion, so
 * nothing rests on a conversion's overflow rule.  0x7f / 0xff (NaN) are never produced.
 */
#ifndef INDEXTTS_HIP_KV8_H
#define INDEXTTS_HIP_KV8_H

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

#endif
