/*
 * indextts_hip_mix.h -- per-row adapter BLENDS of the LoRA adapter bank: the shrink half over weighted mixes of bank voices.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  The Python side lists these entry points as _native.MIX_SYMBOLS; tests/test_lora_mix_cpu.py checks that every
 * prototype below is exported by the library and bound.
 *
 * The bank's identity (indextts_hip.h, itts_lora_shrink) holds for a weighted sum of adapters as it stands:
 *   y = x W + sum_j w_j s_{a_j} (x A_{a_j}^T) B_{a_j}^T = [x | u] [W ; B_bank^T]
 * with u non-zero in the slot of EVERY adapter the row names, each slot scaled by that entry's weight.  The consuming GEMMs, the
 * [W ; B_bank^T] weights and a_bank are those of itts_lora_shrink; only the launch that writes u differs.
 */
#ifndef INDEXTTS_HIP_MIX_H
#define INDEXTTS_HIP_MIX_H

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

/* itts_lora_shrink over mixes.  Every field is that of itts_lora_shrink_args (same layouts, limits and refusals) except `mix`
 * in the place of `ids`:
 *   u[m][a_j * rp + r] = round_T( w_j * sum_k x[m][k] A_bank[a_j][r][k] )   for every non-empty entry j of mix[m]   (r < rp)
 *   every other column of u[m][0 .. Kx) = 0; the padding rows of a packed tail = 0.  ALL Kx columns are written on every call.
 * The sum is accumulated in fp32 in the order of itts_lora_shrink, the weight is applied in fp32, and the product is rounded to T
 * once: a record {a, 1.0f} gives the bits itts_lora_shrink gives for ids[m] = a.  No atomics; the order of a record's entries
 * does not change a bit of the result.
 *   mix     itts_lora_mix_row [M] on the device, read by the kernel: a captured graph serves any assignment of mixes to rows */
typedef struct itts_lora_shrink_mix_args {
  int dtype;
  int M, K;
  const void* x;
  int x_packed, x_mtp;
  const itts_lora_mix_row* mix;
  const void* a_bank;
  int n, rp, Kx;
  void* u;
  int u_packed, u_mtp;
  int64_t ldu;
} itts_lora_shrink_mix_args;
int itts_lora_shrink_mix(const itts_lora_shrink_mix_args* a, void* stream);

#endif
