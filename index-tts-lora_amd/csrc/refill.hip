// The join of continuous batching (itts_refill_join, include/indextts_hip.h): the staged keys / values of the utterances
// that take freed decode slots go into the KV cache, and the entering rows' state -- first token, stop step, own clock, left
// padding, voice record -- into the per-slot tables the captured decode step reads.  One launch between two graph replays, in
// the place of two advanced-index scatters and seven small indexed writes.
#include "common.h"

namespace itts {

constexpr int JOIN_THREADS = 256;

// grid (M + 1, L).  Block (m < M, l): the H * 64 keys and the H * 64 values of staged position m, layer l -- 2 * H << ch_log2
// pieces of 16 bytes, each loaded once (the staging buffers are read once: non-temporal) and stored once by the one thread that
// owns it.  Block (M, 0): the row state, one thread per entering row, and state[2] -= k by thread 0.  The leading arguments are
// flat (pointers first) so that the kernel-argument preload covers what every block needs at once.  Strides are in BYTES here.
__global__ __launch_bounds__(JOIN_THREADS) void refill_join_kernel(
    const char* __restrict__ kst, const char* __restrict__ vst, char* __restrict__ kc, char* __restrict__ vc,
    const int32_t* __restrict__ i_b, const int32_t* __restrict__ i_p, int M, int L, int H, int ch_log2, int n_b, int n_p, int64_t s_l,
    int64_t s_b, int64_t s_h, int64_t s_p, int k, int n_slots, const int32_t* __restrict__ rows, const int32_t* __restrict__ tok,
    const int32_t* __restrict__ fin, const int32_t* __restrict__ stops, const int32_t* __restrict__ pads,
    const B16* __restrict__ mix_new, int step0, int hist_cap, int32_t* __restrict__ tokens, int32_t* __restrict__ history,
    int32_t* __restrict__ finished, int32_t* __restrict__ force_stop, int32_t* __restrict__ row_step0, int32_t* __restrict__ pad,
    B16* __restrict__ mix, int32_t* __restrict__ state) {
  const int m = blockIdx.x, tid = threadIdx.x;
  if (m >= M) {
    if (blockIdx.y != 0) return;
    for (int j = tid; j < k; j += JOIN_THREADS) {
      const int s = rows[j];
      if (s < 0 || s >= n_slots) continue;   // memory guard only: the host deals the slots
      const int t = tok[j];
      tokens[s] = t;
      history[(int64_t)s * hist_cap] = t;
      finished[s] = fin[j];
      force_stop[s] = stops[j];
      row_step0[s] = step0;
      pad[s] = pads[j];
      if (mix != nullptr) {   // the 32-byte voice record of the slot (itts_lora_mix_row)
        st16(mix + 2 * s, ld16<u32x4>(mix_new + 2 * j));
        st16(mix + 2 * s + 1, ld16<u32x4>(mix_new + 2 * j + 1));
      }
    }
    if (tid == 0) state[2] = state[2] - k;   // the entering slots were counted as finished; no other writer between replays
    return;
  }
  const int b = i_b[m], p = i_p[m];
  if (b < 0 || b >= n_b || p < 0 || p >= n_p) return;   // block-uniform
  const int l = blockIdx.y;
  const int per = H << ch_log2;   // pieces of the position's keys (and of its values)
  const int64_t src = ((int64_t)m * L + l) * per * 16;
  const int64_t dst = l * s_l + b * s_b + p * s_p;
  for (int c = tid; c < 2 * per; c += JOIN_THREADS) {
    const bool val = c >= per;
    const int cc = val ? c - per : c;
    const int h = cc >> ch_log2, q = cc & ((1 << ch_log2) - 1);
    const u32x4 v = ld16_nt<u32x4>((val ? vst : kst) + src + (int64_t)cc * 16);
    st16((val ? vc : kc) + dst + h * s_h + q * 16, v);
  }
}

}  // namespace itts

using namespace itts;

extern "C" int itts_refill_join(const itts_refill_join_args* a, void* stream) {
  ITTS_REQUIRE(a, "itts_refill_join: null args");
  const int es = a->dtype == ITTS_F32 ? 4 : (a->dtype == ITTS_BF16 || a->dtype == ITTS_F16) ? 2 : 0;
  ITTS_REQUIRE(es != 0, "itts_refill_join: unknown dtype %d", a->dtype);
  ITTS_REQUIRE(a->M >= 0 && a->k >= 0 && a->L >= 1 && a->L <= 65535 && a->H >= 1, "itts_refill_join: bad shape M=%d k=%d L=%d H=%d",
               a->M, a->k, a->L, a->H);
  ITTS_REQUIRE(a->M == 0 || (a->kst && a->vst && a->kc && a->vc && a->i_b && a->i_p), "itts_refill_join: null cache arguments");
  ITTS_REQUIRE(a->k == 0 || (a->rows && a->tok && a->fin && a->stops && a->pads && a->tokens && a->history && a->finished &&
                             a->force_stop && a->row_step0 && a->pad && a->state),
               "itts_refill_join: null row-state arguments");
  ITTS_REQUIRE((a->mix == nullptr) == (a->mix_new == nullptr), "itts_refill_join: mix and mix_new go together (both or neither)");
  ITTS_REQUIRE(a->n_b >= 0 && a->n_p >= 0 && a->n_slots >= 0 && a->hist_cap >= 1, "itts_refill_join: bad bounds n_b=%d n_p=%d n_slots=%d hist_cap=%d",
               a->n_b, a->n_p, a->n_slots, a->hist_cap);
  const int per16 = 16 / es;   // elements of a 16-byte piece
  ITTS_REQUIRE(a->M == 0 || (a->s_l > 0 && a->s_b > 0 && a->s_h > 0 && a->s_p >= 64 && a->s_l % per16 == 0 && a->s_b % per16 == 0 &&
                             a->s_h % per16 == 0 && a->s_p % per16 == 0),
               "itts_refill_join: the cache strides (elements) must be positive multiples of %d, s_p >= 64", per16);
  ITTS_REQUIRE((((uintptr_t)a->kst | (uintptr_t)a->vst | (uintptr_t)a->kc | (uintptr_t)a->vc | (uintptr_t)a->mix | (uintptr_t)a->mix_new) & 15) == 0,
               "itts_refill_join: kst, vst, kc, vc, mix and mix_new must be 16-byte aligned");
  if (a->M == 0 && a->k == 0) return ITTS_OK;
  const int ch_log2 = es == 4 ? 4 : 3;   // 16-byte pieces of one head's 64 elements: 16 (fp32) or 8
  dim3 grid(a->M + 1, a->L), block(JOIN_THREADS);
  hipLaunchKernelGGL(refill_join_kernel, grid, block, 0, (hipStream_t)stream, (const char*)a->kst, (const char*)a->vst, (char*)a->kc,
                     (char*)a->vc, a->i_b, a->i_p, a->M, a->L, a->H, ch_log2, a->n_b, a->n_p, a->s_l * es, a->s_b * es, a->s_h * es,
                     a->s_p * es, a->k, a->n_slots, a->rows, a->tok, a->fin, a->stops, a->pads, (const B16*)a->mix_new, a->step0,
                     a->hist_cap, a->tokens, a->history, a->finished, a->force_stop, a->row_step0, a->pad, (B16*)a->mix, a->state);
  return check_launch("itts_refill_join");
}
