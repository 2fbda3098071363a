// FP8 (OCP E4M3) KV cache of the paged sampling loop (include/indextts_hip.h).
//   attn_decode_kv8 : the decode step's attention over a one-byte paged pool.  It also APPENDS: the step's QKV GEMM stores
//                     q | k | v row-major (ITTS_EPI_STORE), and the workgroup of a (row, head) quantises that head's new key and
//                     value, stores the 64 + 64 codes at the write position and attends over the pool's keys plus the new one.
//   kv8_store       : the prefill's keys / values, quantised into the pool (one small launch per layer).
// One fp32 power-of-two scale per (layer, K | V, head): k_scale rides on the query's 1/8 factor, v_scale on the final
// normalisation, so the streams are converted code -> f32 and used as they are.
#include "common.h"
#include <type_traits>

namespace itts {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int K8_HD = 64;                // head dim
constexpr int K8_E = 16;                 // codes per lane: one 16-byte request
constexpr int K8_LPR = K8_HD / K8_E;     // lanes per key row: 4
constexpr int K8_RPW = 64 / K8_LPR;      // keys per wave-load: 16 = the smallest cache block, so a request never straddles a block
constexpr int K8_NWV = 4;
constexpr int K8_CH = 4;                 // chunks per wave of a full pass (the 16-bit kernel: 8 chunks of 8 keys)
constexpr int K8_PASS = K8_NWV * K8_RPW * K8_CH;   // 256 keys, as the 16-bit kernel's pass
constexpr float K8_MAX = 448.f;

// 16 values -> 16 codes (dim ascending from the low byte of word 0).  x * inv is exact (inv is a power of two); the clamp comes
// first, so the conversion never sees a value beyond the largest finite code.
__device__ __forceinline__ u32x4 kv8_quant16(const float* x, float inv) {
  u32x4 r;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fminf(fmaxf(x[4 * w + e] * inv, -K8_MAX), K8_MAX);
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], v, true);
    r[w] = (uint32_t)v;
  }
  return r;
}

__device__ __forceinline__ void kv8_decode16(u32x4 c, float* f) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[w], true);
    f[4 * w + 0] = lo[0];
    f[4 * w + 1] = lo[1];
    f[4 * w + 2] = hi[0];
    f[4 * w + 3] = hi[1];
  }
}

// 16 consecutive elements of T -> f32
template <typename T>
__device__ __forceinline__ void kv8_load16(typename Elem<T>::frag a, typename Elem<T>::frag b, float* f) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = Elem<T>::to_f(a[e]);
    f[8 + e] = Elem<T>::to_f(b[e]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Workgroup = (head, row), 4 waves, the launch shape and the request discipline of attn_decode_kernel<T, 4, false, true>
// (attention.hip): everything of a pass is requested before the first use, all K before all V, selects instead of branches, the
// skip word and the context come back in the first trip.  A lane owns 16 dims of a key (16 bytes of codes), 4 lanes a key, a
// wave-load 16 keys; key groups are cut from the left padding rounded down to 16, so a request's block id is wave-uniform.
// The arguments of the first trip lead (14 dwords, preloaded into SGPRs at wave launch); the pools and the output follow.
// The first pass is context-sized: 1..4 chunks per wave for up to 64 / 128 / 192 / 256 key slots.
// The new key (position pos[0]) is not in the pool yet: every lane quantises its 16 dims of the row's new k / v, the decoded codes
// enter the softmax through wave 0's first lane group, and those four lanes store the codes at the end.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(K8_NWV * 64) void attn_decode_kv8_kernel(const T* __restrict__ qkv, const int32_t* __restrict__ pad,
                                                                      const int32_t* __restrict__ pos,
                                                                      const int32_t* __restrict__ skip_rows,
                                                                      const int32_t* __restrict__ kv_tab,
                                                                      const float* __restrict__ kv_scale, int H, int bs_log2,
                                                                      uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                      T* __restrict__ out, int out_mtp) {
  typedef Elem<T> EL;
  typedef typename EL::frag frag;
  constexpr int E = K8_E, LPR = K8_LPR, RPW = K8_RPW, NWV = K8_NWV, CH = K8_CH;
  __shared__ float w_m[NWV], w_l[NWV];
  __shared__ float w_o[NWV][K8_HD];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPR, rg = lane / LPR;
  const int D = H * K8_HD;
  // first trip: the lane's slices of q and of the new k / v, the row's block table, the scalars -- nothing here depends on a
  // loaded value
  const T* row = qkv + (int64_t)b * 3 * D + h * K8_HD + part * E;
  const frag q0 = ld16<frag>(row), q1 = ld16<frag>(row + 8);
  const frag nk0 = ld16<frag>(row + D), nk1 = ld16<frag>(row + D + 8);
  const frag nv0 = ld16<frag>(row + 2 * D), nv1 = ld16<frag>(row + 2 * D + 8);
  const int tabv = kv_tab[b * ITTS_KV_TAB + lane];
  const int bsm = (1 << bs_log2) - 1;
  const int32_t* skip_ptr = skip_rows != nullptr ? skip_rows + b : pos;   // a readable word either way: no branch around the load
  const int skip_raw = *skip_ptr;
  const int j0 = pad[b];
  const float ksc = kv_scale[h], vsc = kv_scale[H + h];
  const bool skipped = skip_rows != nullptr && skip_raw != 0;
  int pos0 = pos[0];
  asm volatile("" : "+s"(pos0));
  asm volatile("" : "+s"(kc), "+s"(vc), "+s"(out));   // the pools and the output (trailing arguments): their scalar load is issued beside the device words, not behind their wait
  const int ctx = skipped ? j0 : pos0;    // pool keys [j0, ctx); the new key is position pos0

  float qf[E], vn[E];
  float sn = 0.f;                         // the new key's score
  u32x4 kcode, vcode;
  float m = -INFINITY, l = 0.f, o[E];
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = 0.f;

  // query conversion and the new key: behind the first pass's requests (or alone, for a row without pool keys)
  auto prep = [&]() {
    float t[E];
    kv8_load16<T>(q0, q1, t);
    const float qs = 0.125f * ksc;
#pragma unroll
    for (int e = 0; e < E; ++e) qf[e] = t[e] * qs;
    kv8_load16<T>(nk0, nk1, t);
    kcode = kv8_quant16(t, 1.0f / ksc);
    kv8_load16<T>(nv0, nv1, t);
    vcode = kv8_quant16(t, 1.0f / vsc);
    kv8_decode16(kcode, t);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) d = fmaf(qf[e], t[e], d);
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) d += __shfl_xor(d, off, 64);
    sn = d;
    kv8_decode16(vcode, vn);
  };

  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  auto key_pass = [&](const int base, auto nch_tag, auto first_tag) {
    constexpr int NCH = decltype(nch_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;
    u32x4 kf[NCH], vf[NCH];
    int64_t eo[NCH];   // byte offset of the lane's codes, the same in the K and in the V pool
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      // first key of this wave-load (wave-uniform); groups past the context fall onto the group of its last key, and the rows past
      // it onto that key (same cache lines, one block; their scores are forced to -inf below)
      const int jf = min(base + (i * NWV + wave_u) * RPW, (ctx - 1) & ~(RPW - 1));
      const int j = min(jf + rg, ctx - 1);
      const int blk = __builtin_amdgcn_readlane(tabv, (jf >> bs_log2) & (ITTS_KV_TAB - 1));
      eo[i] = ((((int64_t)blk * H + h) << bs_log2) + (j & bsm)) * K8_HD + part * E;
      kf[i] = ld16<u32x4>(kc + eo[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NCH; ++i) vf[i] = ld16<u32x4>(vc + eo[i]);
    __builtin_amdgcn_sched_barrier(0);   // every K and V request of the pass is out before anything waits
    if constexpr (FIRST) {
      prep();
      __builtin_amdgcn_sched_barrier(0);
    }
    float sc[NCH];
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      float kx[E];
      kv8_decode16(kf[i], kx);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) d = fmaf(qf[e], kx[e], d);
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) d += __shfl_xor(d, off, 64);
      const int j = base + (i * NWV + wave) * RPW + rg;
      sc[i] = (j >= j0 && j < ctx) ? d : -INFINITY;
      cmax = fmaxf(cmax, sc[i]);
    }
    {
      const float M = fmaxf(m, cmax);
      const float Ms = (M == -INFINITY) ? 0.f : M;
      const float corr = (m == -INFINITY) ? 0.f : __expf(m - Ms);
      l *= corr;
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] *= corr;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const float pv = __expf(sc[i] - Ms);  // -inf -> 0
        l += pv;
        float vx[E];
        kv8_decode16(vf[i], vx);
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = fmaf(pv, vx[e], o[e]);
      }
      m = M;
    }
  };
  typedef std::integral_constant<int, CH> full_t;
  if (j0 < ctx) {
    const int b0 = j0 & ~(RPW - 1);
    // quarter passes the row's key slots [b0, ctx) need, minus one: workgroup-uniform, ONE switch, every arm a straight line
    const int arm = __builtin_amdgcn_readfirstlane(min((ctx - b0 - 1) / (K8_PASS / 4), 3));
    switch (arm) {
      case 0: key_pass(b0, std::integral_constant<int, 1>{}, std::true_type{}); break;
      case 1: key_pass(b0, std::integral_constant<int, 2>{}, std::true_type{}); break;
      case 2: key_pass(b0, std::integral_constant<int, 3>{}, std::true_type{}); break;
      default:
        key_pass(b0, full_t{}, std::true_type{});
        for (int base = b0 + K8_PASS; base < ctx; base += K8_PASS) key_pass(base, full_t{}, std::false_type{});
    }
  } else {
    prep();
  }
  {
    // the new key, through its decoded codes: one more term of the online softmax for wave 0's first lane group (a select)
    const float s1 = (wave == 0 && rg == 0 && !skipped) ? sn : -INFINITY;
    const float M = fmaxf(m, s1);
    const float Ms = (M == -INFINITY) ? 0.f : M;
    const float corr = (m == -INFINITY) ? 0.f : __expf(m - Ms);
    const float pv = __expf(s1 - Ms);
    l = l * corr + pv;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = fmaf(pv, vn[e], o[e] * corr);
    m = M;
  }
  // merge across the key groups of the wave (lanes that share `part`)
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    const float M = fmaxf(m, m2);
    const float sa = (m == -INFINITY) ? 0.f : __expf(m - M);
    const float sb = (m2 == -INFINITY) ? 0.f : __expf(m2 - M);
    l = l * sa + l2 * sb;
    m = M;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float o2 = __shfl_xor(o[e], off, 64);
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
  __syncthreads();
  if (tid < K8_HD && !skipped) {
    float M = w_m[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) M = fmaxf(M, w_m[w]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const float sw = (w_m[w] == -INFINITY) ? 0.f : __expf(w_m[w] - M);
      L += w_l[w] * sw;
      acc += w_o[w][tid] * sw;
    }
    const int64_t oo = out_mtp > 0 ? pa_off<T>(b, h * K8_HD + tid, out_mtp) : ((int64_t)b * H + h) * K8_HD + tid;
    out[oo] = EL::from_f(L > 0.f ? (acc / L) * vsc : 0.f);
    // the append: lanes 0..3 of wave 0 hold the new key's 4 x 16 codes (one owner per element: this workgroup)
    if (tid < LPR) {
      const int blk = kv_tab[b * ITTS_KV_TAB + ((pos0 >> bs_log2) & (ITTS_KV_TAB - 1))];
      const int64_t so = ((((int64_t)blk * H + h) << bs_log2) + (pos0 & bsm)) * K8_HD + tid * E;
      st16(kc + so, kcode);
      st16(vc + so, vcode);
    }
  }
}

// The prefill's K / V of one layer -> codes in the pool.  Thread = 16 dims of (local row, K | V, head) of element blockIdx.y.
template <typename T>
__global__ __launch_bounds__(256) void kv8_store_kernel(const T* __restrict__ qkv, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                        const float* __restrict__ kv_scale, const int32_t* __restrict__ pad,
                                                        const int32_t* __restrict__ row_off,
                                                        const int32_t* __restrict__ cache_shift, int S, int H,
                                                        const int32_t* __restrict__ kv_tab, int bs_log2) {
  typedef typename Elem<T>::frag frag;
  const int b = blockIdx.y;
  const int idx = (int)blockIdx.x * 256 + threadIdx.x;
  const int part = idx & 3, kv = (idx >> 2) & 1, rest = idx >> 3;
  const int h = rest % H, s = rest / H;
  int rbeg = b * S, len = S, p0 = 0, s0 = 0;
  if (row_off != nullptr) {
    rbeg = row_off[b];
    len = min(row_off[b + 1] - rbeg, S);
    p0 = cache_shift != nullptr ? cache_shift[b] : 0;
  } else if (pad != nullptr) {
    s0 = pad[b];
  }
  if (s >= len || s < s0) return;
  const int D = H * K8_HD;
  const T* src = qkv + (int64_t)(rbeg + s) * 3 * D + (int64_t)(1 + kv) * D + h * K8_HD + part * K8_E;
  float t[K8_E];
  kv8_load16<T>(ld16<frag>(src), ld16<frag>(src + 8), t);
  const u32x4 codes = kv8_quant16(t, 1.0f / kv_scale[kv * H + h]);
  const int64_t o = kv_elem_off(kv_tab, bs_log2, b, p0 + s, H, h, 0) + part * K8_E;
  st16((kv ? vc : kc) + o, codes);
}

}  // namespace itts

using namespace itts;

extern "C" int itts_attn_decode_kv8(const void* qkv, void* kcache, void* vcache, void* out, const int32_t* pad, const int32_t* pos,
                                    const float* kv_scale, int B, int H, int dtype, int out_packed, const int32_t* skip_rows,
                                    const int32_t* kv_tab, int kv_bs, void* stream) {
  ITTS_REQUIRE(qkv && kcache && vcache && out && pad && pos && kv_scale && kv_tab, "itts_attn_decode_kv8: null pointer");
  ITTS_REQUIRE(B > 0 && B <= 65535 && H > 0, "itts_attn_decode_kv8: bad shape B=%d H=%d", B, H);
  const int bs_log2 = kv_block_log2(true, kv_bs);
  ITTS_REQUIRE(bs_log2 >= 0, "itts_attn_decode_kv8: kv_bs must be 16, 32 or 64 (got %d)", kv_bs);
  const int out_mtp = out_packed ? (B + 15) / 16 : 0;
  return by_dtype16(dtype, "itts_attn_decode_kv8", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(attn_decode_kv8_kernel<T>, dim3(H, B), dim3(K8_NWV * 64), 0, (hipStream_t)stream, (const T*)qkv,
                       pad, pos, skip_rows, kv_tab, kv_scale, H, bs_log2, (uint8_t*)kcache, (uint8_t*)vcache, (T*)out, out_mtp);
    return check_launch("itts_attn_decode_kv8");
  });
}

extern "C" int itts_kv8_store(const void* qkv, void* kcache, void* vcache, const float* kv_scale, const int32_t* pad,
                              const int32_t* row_off, const int32_t* cache_shift, int B, int S, int H, int dtype,
                              const int32_t* kv_tab, int kv_bs, void* stream) {
  ITTS_REQUIRE(qkv && kcache && vcache && kv_scale && kv_tab, "itts_kv8_store: null pointer");
  ITTS_REQUIRE(B > 0 && B <= 65535 && S > 0 && H > 0 && (int64_t)S * H * 8 < (int64_t)1 << 30, "itts_kv8_store: bad shape B=%d S=%d H=%d",
               B, S, H);
  const int bs_log2 = kv_block_log2(true, kv_bs);
  ITTS_REQUIRE(bs_log2 >= 0, "itts_kv8_store: kv_bs must be 16, 32 or 64 (got %d)", kv_bs);
  return by_dtype16(dtype, "itts_kv8_store", [&](auto tag) {
    using T = typename decltype(tag)::type;
    const int total = S * H * 8;
    hipLaunchKernelGGL(kv8_store_kernel<T>, dim3((total + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, (const T*)qkv,
                       (uint8_t*)kcache, (uint8_t*)vcache, kv_scale, pad, row_off, cache_shift, S, H, kv_tab, bs_log2);
    return check_launch("itts_kv8_store");
  });
}
