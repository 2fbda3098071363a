/*
 * indextts_hip_refill.h -- the JOIN of continuous batching: staged rows enter a running decode loop in one launch.
 *
 * Part of the C ABI (ITTS_ABI_VERSION 9, no struct of indextts_hip.h changed); indextts_hip.h includes it, it is not meant to be
 * included alone.  The Python side lists this entry point as _native.REFILL_SYMBOLS; tests/test_refill_voices_cpu.py checks that
 * the prototype below is exported by the library and bound.
 *
 * Between two replays of the captured decode step, GPTEngine.decode_refill hands the slots of finished rows to new utterances
 * whose prompts were prefilled beside the loop (keys / values kept aside, first token sampled from their own logits).  This
 * launch moves all of it into the loop's buffers: the staged keys and values into the cache, and each entering row's state --
 * with the 32-byte voice record of its slot (indextts_hip_mix.h) -- into the per-slot tables the captured step reads.
 */
#ifndef INDEXTTS_HIP_REFILL_H
#define INDEXTTS_HIP_REFILL_H

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

#endif
