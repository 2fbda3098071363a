// Attention kernels for the GPT-2 decoder (20 heads x 64, scale 1/8, causal, left-pad mask).
//   attn_decode : one query per (batch row, head) over the KV cache -- HBM-bound streaming of K and V.
//   attn_prefill: whole-sequence causal attention (prefill of the decode loop, teacher-forced latent pass).
// Semantics follow HF GPT2Attention as driven by indextts/gpt/model.py:169-182: scores = q.k/sqrt(64), keys visible
// iff causal and attention_mask == 1 (left padding, model.py:643-649); softmax in fp32.
#include "common.h"
#include <type_traits>

namespace itts {

constexpr int HD = 64;  // head dim

// ---------------------------------------------------------------------------------------------------------------------
// Decode: workgroup = (b, h), 4 waves.  Each lane owns a 16-byte slice of a key/value row (8 bf16 / 4 fp32 dims);
// LPR = 64/E lanes cover one row, a wave-load covers RPW = 64/LPR rows (1 KiB, contiguous).  Single pass with online
// softmax: for a pass of NCH row groups per wave the K and then the V fragments are all requested before the first use (one
// memory round trip per pass; a typical 100-300 token context is one pass), every lane keeps a running (max, sum, o[E])
// for the rows it saw, and the partial states are merged across row groups (shuffles) and waves (LDS) at the end.
// The first pass is CONTEXT-SIZED (16-bit types without a row table): NCH in {CH/4, CH/2, 3CH/4, CH} is the smallest that
// covers the row's keys, chosen wave-uniformly once the context is known.  A chunk past the context used to be requested
// anyway, clamped onto the last key: no HBM bytes, but a full 64-lane 16-byte request through the CU's load path, a dot
// product and an exp each, for a term that is exactly zero -- half of all requests at a 75-216 key context.  The
// key-to-lane assignment and every lane's order of operations are those of the full pass: the results are bit-identical.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AD_MAXCTX = 16384;   // validation bound on cache positions per row (nothing in the kernel is sized by it)
constexpr int AD_CH = 8;

__device__ __forceinline__ void softmax_merge(float& m, float& l, float m2, float l2, float& sa, float& sb) {
  float M = fmaxf(m, m2);
  sa = (m == -INFINITY) ? 0.f : __expf(m - M);
  sb = (m2 == -INFINITY) ? 0.f : __expf(m2 - M);
  l = l * sa + l2 * sb;
  m = M;
}

// Diagnostic build only (tools/timeline_attn.py): s_memtime stamps of wave 0 of every workgroup, kept in LDS and written out
// with ordinary vector stores at the end; 16 x u64 per workgroup (linear id = blockIdx.y * gridDim.x + blockIdx.x), see
// include/indextts_hip_diag.h.  A stamp that stands for "this request has landed" WAITS for it (wave 0 only, and only while
// stamps are on): read the shares, the waits forbid overlaps the product kernel has.  The product build gets neither the
// parameter nor an instruction of this.
#if ITTS_DIAG
#define ITTS_AD_DIAG_PARAMS , unsigned long long* __restrict__ stamps, int full_pass
#define ITTS_AD_DIAG_ARGS , itts::g_stamp_buf_attn, itts::g_attn_full_pass
unsigned long long* g_stamp_buf_attn = nullptr;   // (inside namespace itts) itts_debug_set(8, 1) + itts_debug_stamps
int g_attn_full_pass = 0;                         // itts_debug_set(7, 0 | 1)
#else
#define ITTS_AD_DIAG_PARAMS
#define ITTS_AD_DIAG_ARGS
#endif
#if ITTS_STAMPS
#define AD_STAMP(i) ITTS_STAMP_IF(stamps != nullptr, i)
#define AD_STAMP_LANDED(i, cnt)                                              \
  do {                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                       \
    if (stamps != nullptr && threadIdx.x == 0) {                             \
      unsigned long long t_;                                                 \
      asm volatile("s_waitcnt vmcnt(%1)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "n"(cnt) : "memory"); \
      st_[i] = t_;                                                           \
    }                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                       \
  } while (0)
#else
#define AD_STAMP(i) do { } while (0)
#define AD_STAMP_LANDED(i, cnt) do { } while (0)
#endif

// IND: beam search -- key/value position j of logical row b lives in physical cache row kv_rows[parity][b][j] (a table
// that itts_beam_step permutes instead of copying cache rows); parity = *kv_step & 1.
// PAGED: the cache is a block pool behind a per-row block table (include/indextts_hip.h, "Paged KV cache"): lane t of every
// wave keeps table entry t of the row (64 entries, requested with the query), and a key's block id comes out of that
// register with one cross-lane read per K / V request -- no dependent memory access in front of the K / V stream.
// Argument order: the first trip (query, block table, the device words pad / pos / skip / share) needs q, pad, pos, skip_rows,
// kv_share, kv_tab, H and bs_log2 -- 14 dwords, what kernarg preload delivers in SGPRs at wave launch (csrc/Makefile); the caches
// and the output come with a scalar load that the compiler issues behind the device words, beside the query and table requests.
// The row-table form (IND: beam search, not on the benchmarked path) also reads kv_rows, kv_step and rows_total in its first trip;
// they do not fit the 14 dwords and stay in the trailing part, so that form keeps the argument load in front of its table address.
template <typename T, int NWV, bool IND, bool PAGED>
__global__ __launch_bounds__(NWV * 64) void attn_decode_kernel(const T* __restrict__ q, const int32_t* __restrict__ pad,
                                                           const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ skip_rows,
                                                           const int32_t* __restrict__ kv_share,
                                                           const int32_t* __restrict__ kv_tab, int H, int bs_log2,
                                                           const T* __restrict__ kc, const T* __restrict__ vc, int smax,
                                                           T* __restrict__ out, int out_mtp, const int32_t* __restrict__ kv_rows,
                                                           const int32_t* __restrict__ kv_step, int rows_total ITTS_AD_DIAG_PARAMS) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = EL::E;
  constexpr int LPR = HD / E;        // lanes per row: 8 (16-bit) / 16 (fp32)

  constexpr int RPW = 64 / LPR;      // rows per wave-load: 8 / 4
  constexpr int CH = AD_CH * 4 / NWV;   // chunks per wave of a full pass: 4 * RPW * AD_CH keys per workgroup
  constexpr bool SIZED = !IND && sizeof(T) == 2 && CH % 4 == 0;   // context-sized first pass (see above)
  __shared__ float w_m[NWV], w_l[NWV];
  __shared__ float w_o[NWV][HD];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPR, rg = lane / LPR;
#if ITTS_STAMPS
  __shared__ unsigned long long st_[16];
  if (stamps != nullptr && tid < 16) st_[tid] = 0;
  if (stamps != nullptr && tid == 0) st_[14] = __builtin_amdgcn_s_memrealtime();
#endif
  AD_STAMP(0);
  // Two memory round trips, not four: the query fragment and the three device scalars (left padding, cache position, the
  // row's stop flag) are requested together -- nothing here depends on a loaded value -- and the K / V requests follow as
  // soon as the scalars are back; the query is converted only after those have been issued.  (The first version read the
  // stop flag, branched, read pad / pos, waited for q and only then requested K / V: in-kernel latency chain of ~4 trips.)
  const frag qv = ld16<frag>(q + ((int64_t)b * H + h) * HD + part * E);
  int tabv = 0, tab0v = 0;             // PAGED: this row's block table (entry = lane), and row 0's for the shared first keys
  if constexpr (PAGED) {
    tabv = kv_tab[b * ITTS_KV_TAB + lane];
    tab0v = kv_tab[lane];
  }
  const int bsm = (1 << bs_log2) - 1;
  const int32_t* skip_ptr = skip_rows != nullptr ? skip_rows + b : pos;   // a readable word either way: no branch around the load
  const int skip_raw = *skip_ptr;
  const int j0 = pad[b];
  // rows that already emitted their stop token keep decoding only formally (the sampler pads them with the stop token
  // whatever their logits are): their attention -- the one stage whose cost grows with the rows -- is left out: no keys, no
  // requests, no store.  A select, not an early return: a branch here makes the compiler sink the other scalar loads (and the
  // query load) below it, one more round trip each.
  const bool skipped = skip_rows != nullptr && skip_raw != 0;
  // kv_share (one word, (p0 << 8) | C, or NULL / 0): the first C keys of EVERY row ([pad_b, pad_b + C): a one-prompt batch's
  // conditioning latents) hold the same bytes as cache row 0's positions [p0, p0 + C) -- read them there: 32 rows x 20 heads
  // then hit one L2-resident copy instead of streaming 32 copies from HBM (13 % of the K / V bytes at config 3's contexts).
  const int32_t* share_ptr = kv_share != nullptr ? kv_share : pos;     // (a readable word either way, as for skip_rows)
  const int share_raw = *share_ptr;
  const int share_w = (kv_share != nullptr && !IND) ? share_raw : 0;
  const int shC = share_w & 255;
  int pos0 = pos[0];
  asm volatile("" : "+s"(pos0));              // (keeps the load here: the compiler would otherwise load it only for rows that need it)
  // The trailing arguments (kc, vc, smax, out) are NOT pinned here the same way.  The compiler waits for the device words first (a
  // short trip: hot lines), then issues the query and block-table requests together with the trailing arguments' scalar load, and
  // waits for that load in front of the K / V requests: the cold argument trip runs beside the table's.  Pinned beside the device
  // words (measured: profiles/kernarg_preload.txt, "pinned"), the one wait becomes the cold one and the query and table requests
  // queue behind it: 7.91 against 7.35 us per launch, 13 us per token.
  const int ctx = skipped ? j0 : pos0 + 1;    // keys [j0, ctx)
  const int64_t kboff = (PAGED ? 0 : ((int64_t)b * H + h) * smax * HD) + part * E;   // this (row, head)'s keys, the lane's dims
  const int64_t sh_off = ((int64_t)h * smax + (share_w >> 8)) * HD + part * E;   // row 0, head h, position p0
  const int32_t* tab = nullptr;
  if constexpr (IND) tab = kv_rows + ((int64_t)(kv_step[0] & 1) * rows_total + b) * smax;

  AD_STAMP(1);   // trip 1 is back: the context is known

  float qf[E];
  float m = -INFINITY, l = 0.f, o[E];
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = 0.f;

  // one pass over 4 * RPW * AD_CH keys; the FIRST pass (typical contexts need no other) converts the query behind its K / V
  // requests -- written as a separate instance so that the compiler cannot hoist that conversion, and with it the wait for
  // the query, in front of the requests
  // Key groups are cut from a position that is a multiple of RPW (the left padding rounded down; the rows in front of pad_b
  // are masked): a wave-load's RPW consecutive keys then never straddle a cache block (block sizes are multiples of RPW), so
  // in the paged form the block id of a request is WAVE-UNIFORM -- one v_readlane out of the table register per request, no
  // per-lane lookup in front of the K / V stream.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  auto key_pass = [&](const int base, auto nch_tag, auto first_tag) {
    constexpr int NCH = decltype(nch_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;
    frag kf[NCH], vf[NCH];
    int prow[NCH];
    int64_t eo[NCH];   // element offset of the lane's fragment, the same in the K and in the V cache
    // Positions past the context are CLAMPED onto its last key (same cache lines; their scores are forced to -inf below)
    // instead of being skipped: a conditional load is a branch, and a join makes the compiler drain the memory queue.
    if constexpr (IND) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {   // the rows of this chunk's keys, all requested before the first K/V load
        int j = min(base + (i * NWV + wave) * RPW + rg, ctx - 1);
        prow[i] = tab[j];
      }
    }
    int blk0[NCH];   // PAGED with shared first keys: the block of the same key in row 0's window (a per-lane lookup)
    if constexpr (PAGED && !IND) {
      // all of the pass's lookups are issued together, ahead of the address arithmetic: one LDS-crossbar latency for the
      // pass instead of one in front of every request
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int jf = min(base + (i * NWV + wave_u) * RPW, (ctx - 1) & ~(RPW - 1));
        const int ps = (share_w >> 8) + (min(jf + rg, ctx - 1) - j0);
        blk0[i] = __shfl(tab0v, (ps >> bs_log2) & (ITTS_KV_TAB - 1), 64);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      // first key of this wave-load (wave-uniform); groups past the context fall onto the group of its last key, and the rows
      // past it onto that key (same cache lines, one block)
      const int jf = min(base + (i * NWV + wave_u) * RPW, (ctx - 1) & ~(RPW - 1));
      int j = min(jf + rg, ctx - 1);
      int64_t ro = (int64_t)j * HD;
      if constexpr (IND) ro += (int64_t)(prow[i] - b) * H * smax * HD;   // same head, same position, another row
      if constexpr (PAGED) {
        const int blk = __builtin_amdgcn_readlane(tabv, (jf >> bs_log2) & (ITTS_KV_TAB - 1));
        ro = ((((int64_t)blk * H + h) << bs_log2) + (j & bsm)) * HD;
      }
      eo[i] = kboff + ro;
      if constexpr (!IND) {
        const bool sh = (unsigned)(j - j0) < (unsigned)shC;   // a select, not a branch (also false for j < j0: skipped rows)
        int64_t so = sh_off + (int64_t)(j - j0) * HD;
        if constexpr (PAGED) {
          const int ps = (share_w >> 8) + (j - j0);            // the same key in row 0's window
          so = ((((int64_t)blk0[i] * H + h) << bs_log2) + (ps & bsm)) * HD + part * E;
        }
        asm("" : "+v"(so));            // (an opaque value: the compiler would otherwise turn the select into a branch around
                                       //  the table lookup above, a join with an LDS wait in front of every K request)
        eo[i] = sh ? so : eo[i];
      }
      kf[i] = ld16<frag>(kc + eo[i]);
    }
    // All K, then all V: the memory counter retires in order and the softmax needs the maximum over ALL of the pass's scores,
    // so with K and V interleaved the first exp waited for the last-but-one request; now the scores, their shuffles and the
    // maximum run while V is still landing.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NCH; ++i) vf[i] = ld16<frag>(vc + eo[i]);
    __builtin_amdgcn_sched_barrier(0);   // every K AND V request of the pass is out before anything waits
    if constexpr (FIRST) {
#pragma unroll
      for (int e = 0; e < E; ++e) qf[e] = EL::to_f(qv[e]) * 0.125f;
      __builtin_amdgcn_sched_barrier(0);
      AD_STAMP(2);                        // (request order: K0 .. K[NCH-1], V0 .. V[NCH-1])
      AD_STAMP_LANDED(3, 2 * NCH - 1);    // first K
      AD_STAMP_LANDED(4, NCH);            // last K
    }
    float sc[NCH];
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) d = fmaf(qf[e], EL::to_f(kf[i][e]), d);
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) d += __shfl_xor(d, off, 64);
      int j = base + (i * NWV + wave) * RPW + rg;
      sc[i] = (j >= j0 && j < ctx) ? d : -INFINITY;
      cmax = fmaxf(cmax, sc[i]);
    }
    if constexpr (FIRST) AD_STAMP_LANDED(5, 0);   // last V (the scores above ran while it was landing)
    {
      // no branch on "this lane saw a key" (the V fragments would be sunk into it and requested a round trip late): a lane
      // without keys keeps m = -inf and adds zeros
      const float M = fmaxf(m, cmax);
      const float Ms = (M == -INFINITY) ? 0.f : M;
      const float corr = (m == -INFINITY) ? 0.f : __expf(m - Ms);
      l *= corr;
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] *= corr;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        float pv = __expf(sc[i] - Ms);  // -inf -> 0
        l += pv;
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = fmaf(pv, EL::to_f(vf[i][e]), o[e]);
      }
      m = M;
    }
  };
  constexpr int PASS = 4 * RPW * AD_CH;
  typedef std::integral_constant<int, CH> full_t;
  if (j0 < ctx) {
    const int b0 = j0 & ~(RPW - 1);
    // quarter passes the row's key slots [b0, ctx) need, minus one: workgroup-uniform (pad / pos / the skip word are scalars),
    // ONE switch; every arm is the straight line requests -> scores -> softmax, so no request waits behind a join
    int arm = SIZED ? __builtin_amdgcn_readfirstlane(min((ctx - b0 - 1) / (PASS / 4), 3)) : 3;
#if ITTS_DIAG
    if (full_pass) arm = 3;   // itts_debug_set(7, 1): always the full pass (the reference form of tests/test_attn_decode_passes_gpu.py)
#endif
    if constexpr (SIZED) {
      switch (arm) {
        case 0: key_pass(b0, std::integral_constant<int, CH / 4>{}, std::true_type{}); break;
        case 1: key_pass(b0, std::integral_constant<int, CH / 2>{}, std::true_type{}); break;
        case 2: key_pass(b0, std::integral_constant<int, 3 * CH / 4>{}, std::true_type{}); break;
        default:
          key_pass(b0, full_t{}, std::true_type{});
          for (int base = b0 + PASS; base < ctx; base += PASS) key_pass(base, full_t{}, std::false_type{});
      }
    } else {
      key_pass(b0, full_t{}, std::true_type{});
      for (int base = b0 + PASS; base < ctx; base += PASS) key_pass(base, full_t{}, std::false_type{});
    }
#if ITTS_STAMPS
    if (stamps != nullptr && tid == 0) st_[13] = (unsigned long long)((arm + 1) * CH / 4);
#endif
  }
  // merge across the row groups of the wave (lanes that share `part`)
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
    float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    float sa, sb;
    softmax_merge(m, l, m2, l2, sa, sb);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float o2 = __shfl_xor(o[e], off, 64);
      o[e] = o[e] * sa + o2 * sb;
    }
  }
  if (rg == 0) {
#pragma unroll
    for (int e = 0; e < E; ++e) w_o[wave][part * E + e] = o[e];
    if (part == 0) {
      w_m[wave] = m;
      w_l[wave] = l;
    }
  }
  // LDS-only wait + raw barrier: every load of the wave has been consumed by now, and __syncthreads() would also drain vmcnt
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (tid < HD && !skipped) {
    float M = w_m[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) M = fmaxf(M, w_m[w]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      float sw = (w_m[w] == -INFINITY) ? 0.f : __expf(w_m[w] - M);
      L += w_l[w] * sw;
      acc += w_o[w][tid] * sw;
    }
    // out_mtp > 0: packed-activation layout (the out-projection GEMM's operand), else row-major [B][H*64]
    const int64_t o = out_mtp > 0 ? pa_off<T>(b, h * HD + tid, out_mtp) : ((int64_t)b * H + h) * HD + tid;
    AD_STAMP(6);
    out[o] = EL::from_f(L > 0.f ? acc / L : 0.f);
  }
  AD_STAMP(7);
#if ITTS_STAMPS
  if (stamps != nullptr && tid == 0) {
    st_[12] = (unsigned long long)(j0 < ctx ? ctx - (j0 & ~(RPW - 1)) : 0);   // key slots from the first group to the context's end
    st_[15] = __builtin_amdgcn_s_memrealtime();
  }
  // wave 0 wrote every stamp and reads them back: LDS operations of one wave complete in order
  if (stamps != nullptr && tid < 16) stamps[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + tid] = st_[tid];
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// Prefill / latent pass: flash-style causal attention on the matrix cores.  Workgroup = 4 waves = 64 consecutive queries
// of one (b, h); wave w owns 16 query rows.  Per 64-key tile: K rows and a TRANSPOSED V tile are staged in LDS, S = Q K^T
// (A = Q fragments kept in registers, B = K rows: both are 16-byte row-major reads), online softmax in the accumulator
// layout (row max / sum over the 16 lanes that hold a row's columns), P goes through a per-wave LDS scratch to become an
// A operand, O += P V with B = rows of V^T.  fp32 statistics; exact-fp32 MFMA in fp32 mode.  The workgroup whose query
// tile covers a key tile also writes those k/v rows to the cache.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_prefill_kernel(const T* __restrict__ qkv, T* __restrict__ out,
                                                            T* __restrict__ kc, T* __restrict__ vc,
                                                            const int32_t* __restrict__ pad, int S, int H, int smax,
                                                            const int32_t* __restrict__ row_off,
                                                            const int32_t* __restrict__ cache_shift,
                                                            const T* __restrict__ pkc, const T* __restrict__ pvc,
                                                            const int32_t* __restrict__ pre_len,
                                                            const int32_t* __restrict__ pre_row,
                                                            const int32_t* __restrict__ pre_pos0, int pre_qkv,
                                                            T* wkc, T* wvc, const int32_t* __restrict__ w_row,
                                                            const int32_t* __restrict__ w_pos0,
                                                            const int32_t* __restrict__ kv_tab, int bs_log2) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = EL::E, KS = EL::KS, NKS = HD / KS;
  constexpr int ES = (int)sizeof(T);
  constexpr int RS = HD * ES + 16;   // LDS row stride in bytes (64 elements + 16 B pad)
  constexpr int CPR = HD / E;        // 16-byte chunks per row
  __shared__ __attribute__((aligned(16))) unsigned char Ks[64 * RS];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[64 * RS];
  __shared__ __attribute__((aligned(16))) unsigned char Ps[4][16 * RS];
  const int q0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int D = H * HD;
  // packed form (row_off != NULL): the rows of batch element b are [row_off[b], row_off[b+1]) of qkv / out, there is no
  // padding row at all, and cache row = cache_shift[b] + local index (the left-padded cache layout of the decode loop)
  const int rbeg = row_off ? row_off[b] : b * S;
  if (row_off) S = row_off[b + 1] - rbeg;
  if (q0 >= S) return;  // workgroup-uniform
  const int cshift = (row_off && cache_shift) ? cache_shift[b] : 0;
  const int j0 = (pad && !row_off) ? pad[b] : 0;
  const T* base = qkv + (int64_t)rbeg * 3 * D;
  // prefix form (pkc != NULL, packed rows only): the element's sequence is  pl cached keys | its S rows of qkv; only the S
  // rows are queries (query q sits at sequence position pl + q), and key j < pl is read from the cache row pre_row[b] at
  // position pre_pos0[b] + j.  Key tiles are cut from sequence position 0, exactly as if the prefix rows were part of qkv.
  // pre_qkv != 0: the prefix keys are ROWS OF qkv instead (rows pre_pos0[b] .. of the packed buffer: a block that several
  // elements share, computed once in this very pass); pkc / pvc then point at the k / v thirds of qkv.
  // pre_qkv == 2 (append form, contiguous caches only): the prefix is the end of the very cache row this element appends to --
  // row w_row[b], positions [w_pos0[b] - pl, w_pos0[b]); pre_row / pre_pos0 are not read.  The appended positions start at
  // w_pos0[b]: what a launch reads and what it writes never overlap.
  const int pl = pkc != nullptr ? pre_len[b] : 0;
  const bool in_qkv = pre_qkv == 1, cached = pkc != nullptr && !in_qkv;
  // (paged cache: a cached prefix key is addressed through the block table, see kv_elem_off)
  const int p_row = !cached ? 0 : pre_qkv == 2 ? w_row[b] : pre_row[b];
  const int p_pos0 = !cached ? 0 : pre_qkv == 2 ? w_pos0[b] - pl : pre_pos0[b];
  const int64_t pstr = in_qkv ? (int64_t)3 * D : HD;
  const int64_t pbase = pkc == nullptr ? 0
                        : in_qkv       ? (int64_t)pre_pos0[b] * 3 * D + h * HD
                                       : (((int64_t)p_row * H + h) * smax + p_pos0) * HD;
  const int Stot = pl + S;
  // cache append of the prefix form: this workgroup's own 64 rows go to cache row w_row[b], positions w_pos0[b] + local row
  if (wkc != nullptr) {
    const int wr = w_row[b], wp0 = w_pos0[b];
    for (int ch = tid; ch < 64 * CPR; ch += 256) {
      const int kk = ch / CPR, dc = ch - kk * CPR;
      const int q = q0 + kk;
      if (q < S) {
        const T* src = base + (int64_t)q * 3 * D + D + h * HD + dc * E;
        const int64_t o = kv_elem_off(kv_tab, bs_log2, wr, wp0 + q, H, h, smax) + dc * E;
        st16(wkc + o, ld16<frag>(src));
        st16(wvc + o, ld16<frag>(src + D));
      }
    }
  }

  frag qf[NKS];
  {
    const int row = q0 + wave * 16 + c;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      qf[ks] = (row < S) ? ld16<frag>(base + (int64_t)row * 3 * D + h * HD + ks * KS + g * E) : zero_frag<frag>();
  }
  f32x4 O[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) O[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; l[j] = 0.f; }

  const int jend = min(Stot, pl + q0 + 64);
  for (int jt = (j0 / 64) * 64; jt < jend; jt += 64) {
    __syncthreads();
    // ---- stage K rows and V^T (and append to the cache when this workgroup owns the tile)
    for (int ch = tid; ch < 64 * CPR; ch += 256) {
      const int kk = ch / CPR, dc = ch - kk * CPR;
      const int key = jt + kk;
      frag kv = zero_frag<frag>(), vv = zero_frag<frag>();
      if (key < pl) {
        const int64_t po = (kv_tab != nullptr && !in_qkv) ? kv_elem_off(kv_tab, bs_log2, p_row, p_pos0 + key, H, h, smax) + dc * E
                                                           : pbase + (int64_t)key * pstr + dc * E;
        kv = ld16<frag>(pkc + po);
        vv = ld16<frag>(pvc + po);
      } else if (key < Stot) {
        const T* src = base + (int64_t)(key - pl) * 3 * D + D + h * HD + dc * E;
        kv = ld16<frag>(src);
        vv = ld16<frag>(src + D);
        if (kc != nullptr && jt == q0) {
          const int64_t o = kv_elem_off(kv_tab, bs_log2, b, key + cshift, H, h, smax) + dc * E;
          st16(kc + o, kv);
          st16(vc + o, vv);
        }
      }
      st16(Ks + kk * RS + dc * E * ES, kv);
#pragma unroll
      for (int e = 0; e < E; ++e) *reinterpret_cast<T*>(Vt + (dc * E + e) * RS + kk * ES) = vv[e];
    }
    __syncthreads();
    if (jt + 64 <= j0) continue;  // tile entirely inside the left padding (block-uniform)
    // ---- S = Q K^T  (per wave: 16 queries x 64 keys)
    f32x4 sacc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      sacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        frag bf = ld16<frag>(Ks + (16 * n + c) * RS + (ks * KS + g * E) * ES);
        sacc[n] = EL::mma(qf[ks], bf, sacc[n]);
      }
    }
    // ---- online softmax; this lane holds rows 4g+j (j<4), columns 16n+c (n<4)
    float rmax[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = pl + q0 + wave * 16 + 4 * g + j;   // sequence position of the query
      float mx = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int key = jt + 16 * n + c;
        const bool vis = (key <= q) && (key >= j0) && (key < Stot);
        const float v = vis ? sacc[n][j] * 0.125f : -INFINITY;
        sacc[n][j] = v;
        mx = fmaxf(mx, v);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      rmax[j] = mx;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mn = fmaxf(m[j], rmax[j]);
      const float corr = (m[j] == -INFINITY) ? 0.f : __expf(m[j] - mn);
      float rs = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float pv = (sacc[n][j] == -INFINITY) ? 0.f : __expf(sacc[n][j] - mn);
        sacc[n][j] = pv;
        rs += pv;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
      l[j] = l[j] * corr + rs;
      m[j] = mn;
#pragma unroll
      for (int n = 0; n < 4; ++n) O[n][j] *= corr;
    }
    // ---- P: accumulator layout -> A-operand layout through the wave's LDS scratch
    unsigned char* ps = Ps[wave];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<T*>(ps + (4 * g + j) * RS + (16 * n + c) * ES) = EL::from_f(sacc[n][j]);
    // same wave wrote and reads: LDS operations of a wave complete in order, no barrier needed
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      frag af = ld16<frag>(ps + c * RS + (ks * KS + g * E) * ES);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        frag bf = ld16<frag>(Vt + (16 * n + c) * RS + (ks * KS + g * E) * ES);
        O[n] = EL::mma(af, bf, O[n]);
      }
    }
  }
  // ---- normalise and store: rows 4g+j, dims 16n+c
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = q0 + wave * 16 + 4 * g + j;
    if (q >= S) continue;
    const float inv = l[j] > 0.f ? 1.0f / l[j] : 0.f;
    T* orow = out + ((int64_t)rbeg + q) * D + h * HD;
#pragma unroll
    for (int n = 0; n < 4; ++n) orow[16 * n + c] = EL::from_f(O[n][j] * inv);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Append form, narrow query tile (the incremental latent pass of a stream: 1-64 new rows behind several hundred cached keys).
// Workgroup = 16 consecutive queries of one (element, head) -- ONE MFMA row block -- and still 4 waves: at a chunk of 16 the
// 64-query tile above has three of its four waves multiplying zero queries, and only H x E workgroups exist.  Here the waves
// share one query block and split the COLUMNS of both products: wave w computes the score block of keys 16w .. 16w+15 of the
// tile (sacc[w] of the kernel above) and the output block of head dims 16w .. 16w+15 (O[w] above).  The raw score blocks are
// exchanged through LDS (Ss), after which every wave holds all four and runs the SAME online softmax the kernel above runs --
// four times redundantly, 16 exps per lane per tile, which is cheaper than a second exchange.  Every chain of a query row (the
// ks order inside sacc[n] and O[n], the n order of the row sum, the 16-lane shuffles, the scale 0.125, the tile order from
// sequence position 0) is the one of attn_prefill_kernel, so a row's bits do not depend on the form.  A tile whose keys are all
// behind a query leaves that row's state untouched (corr = 1, p = 0), so the tiles the 64-query form walks past a row's own
// position, and this form does not, change nothing either.
// Staging: all 256 threads stage the 64-key tile (K rows, V transposed); the NEXT tile's 16-byte requests are issued into
// registers right after the current tile is in LDS and land while the MFMAs and the softmax run (the barrier of the score
// exchange waits for LDS only, not for those requests).
// Contiguous caches only: the prefix of element e is cache row w_row[e], positions [w_pos0[e] - pre_len[e], w_pos0[e]); the own
// rows' k / v are stored at w_pos0[e] + local row, and as keys they are taken from qkv, never read back.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_append16_kernel(const T* __restrict__ qkv, T* __restrict__ out, T* kc, T* vc,
                                                             const int32_t* __restrict__ row_off,
                                                             const int32_t* __restrict__ pre_len,
                                                             const int32_t* __restrict__ w_row,
                                                             const int32_t* __restrict__ w_pos0, int H, int smax) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = EL::E, KS = EL::KS, NKS = HD / KS;
  constexpr int ES = (int)sizeof(T);
  constexpr int RS = HD * ES + 16;        // LDS row stride in bytes (64 elements + 16 B pad), as above
  constexpr int CPR = HD / E;             // 16-byte chunks per row
  constexpr int NCH = 64 * CPR / 256;     // chunks of a 64-key tile per thread: 2 (16-bit) / 4 (fp32)
  constexpr int SS = 68;                  // floats per Ss row: the four row groups of a lane quad land 16 banks apart
  __shared__ __attribute__((aligned(16))) unsigned char Ks[64 * RS];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[64 * RS];
  __shared__ __attribute__((aligned(16))) unsigned char Ps[4][16 * RS];
  __shared__ float Ss[16 * SS];
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int D = H * HD;
  const int rbeg = row_off[b];
  const int S = row_off[b + 1] - rbeg;
  if (q0 >= S) return;  // workgroup-uniform
  const int pl = pre_len[b], wr = w_row[b], wp0 = w_pos0[b];
  const int Stot = pl + S;
  const T* base = qkv + (int64_t)rbeg * 3 * D;
  const int64_t crow = ((int64_t)wr * H + h) * smax * HD;   // this (cache row, head)
  const int64_t pbase = crow + (int64_t)(wp0 - pl) * HD;    // prefix key j sits at pbase + j * 64

  // ---- append this workgroup's own 16 rows
  if (tid < 16 * CPR) {
    const int kk = tid / CPR, dc = tid - kk * CPR;
    const int q = q0 + kk;
    if (q < S) {
      const T* src = base + (int64_t)q * 3 * D + D + h * HD + dc * E;
      const int64_t o = crow + (int64_t)(wp0 + q) * HD + dc * E;
      st16(kc + o, ld16<frag>(src));
      st16(vc + o, ld16<frag>(src + D));
    }
  }

  frag qf[NKS];
  {
    const int row = q0 + c;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      qf[ks] = (row < S) ? ld16<frag>(base + (int64_t)row * 3 * D + h * HD + ks * KS + g * E) : zero_frag<frag>();
  }
  f32x4 O = f32x4{0.f, 0.f, 0.f, 0.f};   // rows 4g+j, head dim 16*wave + c
  float m[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; l[j] = 0.f; }

  frag kr[NCH], vr[NCH];
  auto request_tile = [&](const int jt) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * 256;
      const int kk = ch / CPR, dc = ch - kk * CPR;
      const int key = jt + kk;
      kr[i] = zero_frag<frag>();
      vr[i] = zero_frag<frag>();
      if (key < pl) {
        const int64_t po = pbase + (int64_t)key * HD + dc * E;
        kr[i] = ld16<frag>(kc + po);
        vr[i] = ld16<frag>(vc + po);
      } else if (key < Stot) {
        const T* src = base + (int64_t)(key - pl) * 3 * D + D + h * HD + dc * E;
        kr[i] = ld16<frag>(src);
        vr[i] = ld16<frag>(src + D);
      }
    }
  };

  const int jend = min(Stot, pl + q0 + 16);
  request_tile(0);
  for (int jt = 0; jt < jend; jt += 64) {
    __syncthreads();   // the last tile's readers are done (and the requested fragments have landed)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * 256;
      const int kk = ch / CPR, dc = ch - kk * CPR;
      st16(Ks + kk * RS + dc * E * ES, kr[i]);
#pragma unroll
      for (int e = 0; e < E; ++e) *reinterpret_cast<T*>(Vt + (dc * E + e) * RS + kk * ES) = vr[i][e];
    }
    __syncthreads();
    if (jt + 64 < jend) request_tile(jt + 64);   // workgroup-uniform; in flight until the next iteration's first barrier
    // ---- this wave's block of S = Q K^T: 16 queries x keys 16*wave .. 16*wave + 15
    {
      f32x4 sw = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        frag bf = ld16<frag>(Ks + (16 * wave + c) * RS + (ks * KS + g * E) * ES);
        sw = EL::mma(qf[ks], bf, sw);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) Ss[(4 * g + j) * SS + 16 * wave + c] = sw[j];
    }
    // LDS-only wait + raw barrier: __syncthreads() would also wait for the next tile's requests
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    f32x4 sacc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) sacc[n][j] = Ss[(4 * g + j) * SS + 16 * n + c];
    // ---- online softmax, as in attn_prefill_kernel; this lane holds rows 4g+j (j<4), columns 16n+c (n<4)
    float rmax[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = pl + q0 + 4 * g + j;   // sequence position of the query
      float mx = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int key = jt + 16 * n + c;
        const bool vis = (key <= q) && (key < Stot);
        const float v = vis ? sacc[n][j] * 0.125f : -INFINITY;
        sacc[n][j] = v;
        mx = fmaxf(mx, v);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      rmax[j] = mx;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mn = fmaxf(m[j], rmax[j]);
      const float corr = (m[j] == -INFINITY) ? 0.f : __expf(m[j] - mn);
      float rs = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float pv = (sacc[n][j] == -INFINITY) ? 0.f : __expf(sacc[n][j] - mn);
        sacc[n][j] = pv;
        rs += pv;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
      l[j] = l[j] * corr + rs;
      m[j] = mn;
      O[j] *= corr;
    }
    // ---- P: accumulator layout -> A-operand layout through the wave's own LDS scratch (same wave writes and reads)
    unsigned char* ps = Ps[wave];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<T*>(ps + (4 * g + j) * RS + (16 * n + c) * ES) = EL::from_f(sacc[n][j]);
    // ---- this wave's block of O += P V: head dims 16*wave .. 16*wave + 15
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      frag af = ld16<frag>(ps + c * RS + (ks * KS + g * E) * ES);
      frag bf = ld16<frag>(Vt + (16 * wave + c) * RS + (ks * KS + g * E) * ES);
      O = EL::mma(af, bf, O);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = q0 + 4 * g + j;
    if (q >= S) continue;
    const float inv = l[j] > 0.f ? 1.0f / l[j] : 0.f;
    out[((int64_t)rbeg + q) * D + h * HD + 16 * wave + c] = EL::from_f(O[j] * inv);
  }
}

}  // namespace itts

using namespace itts;

#if ITTS_DIAG
namespace itts { int g_attn_waves = 4; }  // diagnostic build: itts_debug_set(4, 4|8) waves per decode-attention workgroup
#else
namespace itts { constexpr int g_attn_waves = 4; }  // measured equal to 8; the 8-wave instantiation folds away
#endif

extern "C" int itts_attn_decode(const void* q, const void* kcache, const void* vcache, void* out, const int32_t* pad,
                                const int32_t* pos, int B, int H, int smax, int dtype, int out_packed, const int32_t* kv_rows,
                                const int32_t* kv_step, const int32_t* skip_rows, const int32_t* kv_share, const int32_t* kv_tab,
                                int kv_bs, void* stream) {
  const int out_mtp = out_packed ? (B + 15) / 16 : 0;
  ITTS_REQUIRE(q && kcache && vcache && out && pad && pos, "itts_attn_decode: null pointer");
  const bool paged = kv_tab != nullptr;
  ITTS_REQUIRE(B > 0 && H > 0 && (paged || (smax > 0 && smax <= AD_MAXCTX)), "itts_attn_decode: bad shape B=%d H=%d smax=%d (max %d)", B, H,
               smax, AD_MAXCTX);
  const int bs_log2 = kv_block_log2(paged, kv_bs);
  ITTS_REQUIRE(bs_log2 >= 0 && (!paged || kv_rows == nullptr),
               "itts_attn_decode: a paged cache needs kv_bs in {16, 32, 64} and no beam row table");
  ITTS_REQUIRE((kv_rows == nullptr) == (kv_step == nullptr), "itts_attn_decode: pass both or neither of kv_rows / kv_step");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(H, B), block(g_attn_waves * 64);
  const bool ind = kv_rows != nullptr;
  return by_dtype(dtype, "itts_attn_decode", [&](auto tag) {
    using T = typename decltype(tag)::type;
#define ITTS_AD(NW_, IND_, PG_)                                                                                                   \
  hipLaunchKernelGGL((attn_decode_kernel<T, NW_, IND_, PG_>), grid, block, 0, s, (const T*)q, pad, pos, skip_rows, kv_share, kv_tab, H, \
                     bs_log2, (const T*)kcache, (const T*)vcache, smax, (T*)out, out_mtp, kv_rows, kv_step, B ITTS_AD_DIAG_ARGS)
    if (paged) { if (g_attn_waves == 8) ITTS_AD(8, false, true); else ITTS_AD(4, false, true); }
    else if (g_attn_waves == 8) { if (ind) ITTS_AD(8, true, false); else ITTS_AD(8, false, false); }
    else { if (ind) ITTS_AD(4, true, false); else ITTS_AD(4, false, false); }
#undef ITTS_AD
    return check_launch("itts_attn_decode");
  });
}

static int attn_prefill_impl(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* pad, int B, int S, int H,
                             int smax, int dtype, const int32_t* row_off, const int32_t* cache_shift, void* stream,
                             const void* pkc = nullptr, const void* pvc = nullptr, const int32_t* pre_len = nullptr,
                             const int32_t* pre_row = nullptr, const int32_t* pre_pos0 = nullptr, int pre_qkv = 0,
                             void* wkc = nullptr, void* wvc = nullptr, const int32_t* w_row = nullptr,
                             const int32_t* w_pos0 = nullptr, const int32_t* kv_tab = nullptr, int kv_bs = 0) {
  ITTS_REQUIRE(qkv && out, "itts_attn_prefill: null pointer");
  const int bs_log2 = kv_block_log2(kv_tab != nullptr, kv_bs);
  ITTS_REQUIRE(bs_log2 >= 0, "itts_attn_prefill: kv_bs must be 16, 32 or 64");
  if (kv_tab != nullptr && kcache != nullptr) smax = S > smax ? S : smax;   // (no per-row capacity in the paged form)
  ITTS_REQUIRE((kcache == nullptr) == (vcache == nullptr), "itts_attn_prefill: pass both caches or neither");
  ITTS_REQUIRE(B > 0 && S > 0 && H > 0 && (!kcache || S <= smax), "itts_attn_prefill: bad shape B=%d S=%d H=%d smax=%d", B, S, H, smax);
  ITTS_REQUIRE(B <= 65535 && H <= 65535, "itts_attn_prefill: grid too large");
  dim3 grid((S + 63) / 64, H, B), block(256);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, "itts_attn_prefill", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(attn_prefill_kernel<T>, grid, block, 0, s, (const T*)qkv, (T*)out, (T*)kcache, (T*)vcache, pad, S, H, smax, row_off,
                       cache_shift, (const T*)pkc, (const T*)pvc, pre_len, pre_row, pre_pos0, pre_qkv, (T*)wkc, (T*)wvc, w_row, w_pos0,
                       kv_tab, bs_log2);
    return check_launch("itts_attn_prefill");
  });
}

extern "C" int itts_attn_prefill(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* pad, int B, int S,
                                 int H, int smax, int dtype, void* stream) {
  return attn_prefill_impl(qkv, out, kcache, vcache, pad, B, S, H, smax, dtype, nullptr, nullptr, stream);
}

extern "C" int itts_attn_prefill_prefix(const void* qkv, void* out, const void* kcache, const void* vcache, const int32_t* row_off,
                                        const int32_t* pre_len, const int32_t* pre_row, const int32_t* pre_pos0, int B, int Smax,
                                        int H, int smax, int dtype, const int32_t* kv_tab, int kv_bs, void* stream) {
  ITTS_REQUIRE(row_off && kcache && vcache && pre_len && pre_row && pre_pos0, "itts_attn_prefill_prefix: null pointer");
  return attn_prefill_impl(qkv, out, nullptr, nullptr, nullptr, B, Smax, H, smax, dtype, row_off, nullptr, stream, kcache, vcache,
                           pre_len, pre_row, pre_pos0, 0, nullptr, nullptr, nullptr, nullptr, kv_tab, kv_bs);
}

// itts_attn_prefill_shared with pre_row0 == NULL: the cached-prefix append form (include/indextts_hip.h).  Two kernel forms, the
// same bits per row: chunks (Smax <= ATTN_APPEND_NARROW_MAX) take the 16-query tile, longer passes -- a stream's first one carries
// the prompt -- the 64-query tile of attn_prefill_kernel, which stages every key tile once per 64 queries instead of once per 16.
constexpr int ATTN_APPEND_NARROW_MAX = 128;

static int attn_append_impl(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* row_off, const int32_t* pre_len,
                            const int32_t* w_row, const int32_t* w_pos0, int E, int Smax, int H, int smax, int dtype,
                            const int32_t* kv_tab, void* stream) {
  ITTS_REQUIRE(qkv && out && row_off && pre_len && kcache && vcache && w_row && w_pos0,
               "itts_attn_prefill_shared (append form): null pointer (qkv, out, row_off, pre_len, both caches, w_row and w_pos0 are required)");
  ITTS_REQUIRE(kv_tab == nullptr, "itts_attn_prefill_shared (append form): a paged cache (kv_tab) is not supported, pass contiguous caches");
  ITTS_REQUIRE(E > 0 && E <= 65535 && H > 0 && H <= 65535 && Smax >= 1 && smax >= 1 && Smax <= smax,
               "itts_attn_prefill_shared (append form): bad shape E=%d Smax=%d H=%d smax=%d", E, Smax, H, smax);
  if (Smax > ATTN_APPEND_NARROW_MAX) {
    const int rc = attn_prefill_impl(qkv, out, nullptr, nullptr, nullptr, E, Smax, H, smax, dtype, row_off, nullptr, stream, kcache, vcache,
                                     pre_len, pre_len /* unused */, pre_len /* unused */, 2, kcache, vcache, w_row, w_pos0, nullptr, 0);
    if (rc == ITTS_OK) set_last_kernel("attn_append<64>");
    return rc;
  }
  dim3 grid((Smax + 15) / 16, H, E), block(256);
  return by_dtype(dtype, "itts_attn_prefill_shared", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(attn_append16_kernel<T>, grid, block, 0, (hipStream_t)stream, (const T*)qkv, (T*)out, (T*)kcache, (T*)vcache,
                       row_off, pre_len, w_row, w_pos0, H, smax);
    set_last_kernel("attn_append<16>");
    return check_launch("itts_attn_prefill_shared");
  });
}

extern "C" int itts_attn_prefill_shared(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* row_off,
                                        const int32_t* pre_len, const int32_t* pre_row0, const int32_t* w_row,
                                        const int32_t* w_pos0, int E, int Smax, int H, int smax, int dtype, const int32_t* kv_tab,
                                        int kv_bs, void* stream) {
  if (pre_row0 == nullptr) return attn_append_impl(qkv, out, kcache, vcache, row_off, pre_len, w_row, w_pos0, E, Smax, H, smax, dtype,
                                                   kv_tab, stream);
  ITTS_REQUIRE(qkv && row_off && pre_len && pre_row0 && (kcache == nullptr) == (vcache == nullptr) &&
                   (kcache == nullptr || (w_row && w_pos0)), "itts_attn_prefill_shared: null pointer");
  const int D = H * 64;
  const int es = dtype == ITTS_F32 ? 4 : 2;
  const char* q = (const char*)qkv;
  return attn_prefill_impl(qkv, out, nullptr, nullptr, nullptr, E, Smax, H, smax, dtype, row_off, nullptr, stream,
                           q + (int64_t)D * es, q + (int64_t)2 * D * es, pre_len, pre_len /* unused */, pre_row0, 1, kcache, vcache,
                           w_row, w_pos0, kv_tab, kv_bs);
}

extern "C" int itts_attn_prefill_packed(const void* qkv, void* out, void* kcache, void* vcache, const int32_t* row_off,
                                        const int32_t* cache_shift, int B, int Smax, int H, int smax, int dtype,
                                        const int32_t* kv_tab, int kv_bs, void* stream) {
  ITTS_REQUIRE(row_off, "itts_attn_prefill_packed: row_off is null");
  return attn_prefill_impl(qkv, out, kcache, vcache, nullptr, B, Smax, H, smax, dtype, row_off, cache_shift, stream, nullptr, nullptr,
                           nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, kv_tab, kv_bs);
}

// ---------------------------------------------------------------------------------------------------------------
// A one-prompt batch's shared rows (the conditioning latents) are computed once by the packed prefill and land in cache row 0;
// this copies their keys / values, all layers in one launch, to the same sequence positions of every other row:
//   row b, positions [pad[b], pad[b] + C)  <-  row 0, positions [p0, p0 + C)          (b = 1 .. B-1; 16 bytes per thread)
// Both cache forms (kv_tab NULL: contiguous rows).  Replaces two advanced-indexing gathers and two scatters of the torch form.
// ---------------------------------------------------------------------------------------------------------------
namespace itts {
__global__ __launch_bounds__(256) void kv_share_rows_kernel(char* __restrict__ kc, char* __restrict__ vc, int64_t layer_bytes, int H, int C,
                                                            int p0, const int32_t* __restrict__ pad, int smax,
                                                            const int32_t* __restrict__ kv_tab, int bs_log2, int es, int total) {
  const int idx = (int)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cpr = 64 * es / 16;                        // 16-byte chunks of a 64-element row: 8 (16-bit) / 16 (fp32)
  const int seg = idx % cpr, kv = (idx / cpr) & 1, rest = idx / (2 * cpr);
  const int c = rest % C, h = rest / C;
  const int b = (int)blockIdx.y + 1;
  char* base = (kv ? vc : kc) + (int64_t)blockIdx.z * layer_bytes;
  const int64_t so = kv_elem_off(kv_tab, bs_log2, 0, p0 + c, H, h, smax) * es + seg * 16;
  const int64_t d_o = kv_elem_off(kv_tab, bs_log2, b, pad[b] + c, H, h, smax) * es + seg * 16;
  st16(base + d_o, ld16<B16>(base + so));
}
}  // namespace itts

extern "C" int itts_kv_share_rows(void* kcache, void* vcache, int layers, int64_t layer_stride, int B, int H, int C, int p0,
                                  const int32_t* pad, int smax, const int32_t* kv_tab, int kv_bs, int dtype, void* stream) {
  ITTS_REQUIRE(kcache && vcache && pad && layers > 0 && B >= 1 && H > 0 && C > 0 && p0 >= 0, "itts_kv_share_rows: bad arguments");
  const int bs_log2 = kv_block_log2(kv_tab != nullptr, kv_bs);
  ITTS_REQUIRE(bs_log2 >= 0 && (kv_tab != nullptr || smax >= p0 + C),
               "itts_kv_share_rows: paged cache: kv_bs must be 16, 32 or 64; contiguous cache: smax covers the block");
  ITTS_REQUIRE(layers <= 65535 && B <= 65536, "itts_kv_share_rows: too many layers / rows");
  if (B == 1) return ITTS_OK;   // (nothing to copy: like the M == 0 returns elsewhere, in front of the dtype dispatch)
  return by_dtype(dtype, "itts_kv_share_rows", [&](auto tag) {   // one kernel moves 16-byte chunks: only the element size matters
    const int es = (int)sizeof(typename decltype(tag)::type);
    const int total = H * C * 2 * (64 * es / 16);
    hipLaunchKernelGGL(itts::kv_share_rows_kernel, dim3((total + 255) / 256, B - 1, layers), dim3(256), 0, (hipStream_t)stream,
                       (char*)kcache, (char*)vcache, layer_stride * es, H, C, p0, pad, smax, kv_tab, bs_log2, es, total);
    return check_launch("itts_kv_share_rows");
  });
}
