// FP8 (OCP e4m3) KV cache: the quantising append and the split-KV decode
// attention over one-byte keys and values (ops/llm.py: rope_kv_append,
// rope_kv_extend and attention_decode on torch.float8_e4m3fn caches).
//
// Caches are e4m3 [B][Hkv][max_len][D], decode.hip's layout at one byte per
// element.  kv_scale is fp32 [4][Hkv]: rows k_scale, v_scale, 1/k_scale,
// 1/v_scale (the reciprocals are computed once on the host side, so this file
// and the torch rule multiply by the same bits).
//
//   byte = e4m3_rne(clamp(float(x_bf16) * inv_scale, -448, 448))
//
// x_bf16 is the rotated key rounded to bf16 as k_rope rounds it, or the V
// head as it is.  The clamp comes first, so the convert never sees a value it
// would have to saturate.  NaN / inf inputs: unspecified.
//
// attn_decode_fp8 keeps decode.hip's main loop (global memory -> VGPRs, VALU
// dot products, no LDS, no barrier, fp32 online softmax in exp2 form, fixed
// fold order, no float atomics) and is laid out for one-byte elements: a
// 16-byte load is 16 elements, a key is D/16 lanes, one load instruction of a
// wave covers twice the keys, and the key tile is 128 so a lane has as many
// 16-byte loads in flight per tile as the bf16 kernel (4 K + 4 V at D = 128).
// k_scale * D^-0.5 * log2e is folded into the fp32 query once; v_scale
// multiplies the block's merged accumulator once.  G = 8 would need 2 * 8 * 16
// query and accumulator registers that way, so it takes 8-byte loads (8
// elements per lane, D/8 lanes per key, twice the loads per tile).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef float f8_f32x2 __attribute__((ext_vector_type(2)));

constexpr int NT = 256;
constexpr int KT8 = 128;  // keys per tile

__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ float bf2f(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// 4 e4m3 bytes -> 4 floats (v_cvt_pk_f32_fp8, low and high half)
__device__ __forceinline__ void unpack4(uint32_t w, float* v) {
  const f8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  v[0] = a[0];
  v[1] = a[1];
  v[2] = b[0];
  v[3] = b[1];
}

__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }

// 4 bf16 values -> 4 e4m3 bytes by the rule above (v_cvt_pk_fp8_f32 rounds to nearest even)
__device__ __forceinline__ uint32_t quant4(const uint16_t* x, float inv) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(bf2f(x[0]) * inv), clamp448(bf2f(x[1]) * inv), 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(bf2f(x[2]) * inv), clamp448(bf2f(x[3]) * inv), r, true);
  return (uint32_t)r;
}

__device__ __forceinline__ void split8(const uint4 q, uint16_t* v) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = (uint16_t)(w[i] & 0xffffu);
    v[2 * i + 1] = (uint16_t)(w[i] >> 16);
  }
}

__device__ __forceinline__ uint4 join8(const uint16_t* v) {
  return uint4{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
               (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16)};
}

// ---------------------------------------------------------------- rope_kv_extend_fp8
// qkv row b*T + t = [H q heads | Hkv k heads | Hkv v heads] x D bf16 of new
// token t of batch row b, p = lens[b] + t its position (n_new == nullptr:
// every t < T counts, the decode append at T = 1).  Liveness is
// k_rope_kv_extend's: a token with t >= n_new[b] or p outside [0, min(max_len,
// table_len)) writes nothing and its q columns are left alone.  The rotation
// is k_rope's arithmetic (llm_kernels.hip), expression for expression, on 8
// rotate_half pairs (i, i + D/2) per thread, so a thread owns 8 consecutive
// cache bytes in each half of the head: the q heads go back in place as bf16,
// the rotated K head and the V head are quantised and leave as 8-byte stores.
__global__ __launch_bounds__(NT) void k_rope_kv_extend_fp8(uint16_t* qkv, const float* __restrict__ cs,
                                                           const float* __restrict__ sn, uint8_t* __restrict__ kc,
                                                           uint8_t* __restrict__ vc, const float* __restrict__ kv_scale,
                                                           const int* __restrict__ lens, const int* __restrict__ n_new,
                                                           int B, int T, int H, int Hkv, int D, int max_len,
                                                           int table_len, float sign) {
  const int H2 = D >> 1, Q = H2 >> 3;
  const int nh = H + 2 * Hkv;
  const long long total = (long long)B * T * nh * Q;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int q = (int)(i % Q);
    const long long r = i / Q;
    const int hd = (int)(r % nh);
    const long long bt = r / nh;
    const int b = (int)(bt / T), t = (int)(bt % T);
    const long long pl = (long long)lens[b] + t;
    if ((n_new && t >= n_new[b]) || pl < 0 || pl >= max_len || pl >= table_len) continue;
    const int p = (int)pl;
    const long long off = bt * nh * D + (long long)hd * D + q * 8;
    uint16_t x1[8], x2[8];
    split8(*reinterpret_cast<const uint4*>(qkv + off), x1);
    split8(*reinterpret_cast<const uint4*>(qkv + off + H2), x2);
    if (hd >= H + Hkv) {  // v head: quantised as it is
      const int g = hd - H - Hkv;
      const float inv = kv_scale[3 * Hkv + g];
      uint8_t* base = vc + (((long long)b * Hkv + g) * max_len + p) * D + q * 8;
      *reinterpret_cast<uint2*>(base) = uint2{quant4(x1, inv), quant4(x1 + 4, inv)};
      *reinterpret_cast<uint2*>(base + H2) = uint2{quant4(x2, inv), quant4(x2 + 4, inv)};
      continue;
    }
    uint16_t o1[8], o2[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const float4 c = *reinterpret_cast<const float4*>(cs + (long long)p * H2 + q * 8 + half * 4);
      const float4 n = *reinterpret_cast<const float4*>(sn + (long long)p * H2 + q * 8 + half * 4);
      const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sign * n.x, sign * n.y, sign * n.z, sign * n.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a1 = bf2f(x1[half * 4 + e]), a2 = bf2f(x2[half * 4 + e]);
        o1[half * 4 + e] = f2bf(a1 * cc[e] - a2 * ss[e]);
        o2[half * 4 + e] = f2bf(a2 * cc[e] + a1 * ss[e]);
      }
    }
    if (hd < H) {  // q head: rotated in place
      *reinterpret_cast<uint4*>(qkv + off) = join8(o1);
      *reinterpret_cast<uint4*>(qkv + off + H2) = join8(o2);
      continue;
    }
    const int g = hd - H;
    const float inv = kv_scale[2 * Hkv + g];
    uint8_t* base = kc + (((long long)b * Hkv + g) * max_len + p) * D + q * 8;
    *reinterpret_cast<uint2*>(base) = uint2{quant4(o1, inv), quant4(o1 + 4, inv)};
    *reinterpret_cast<uint2*>(base + H2) = uint2{quant4(o2, inv), quant4(o2 + 4, inv)};
  }
}

// ---------------------------------------------------------------- attn_decode_fp8
// Grid (n_splits, Hkv, B), 256 threads.  Block (s, g, b) owns the keys
// [s*chunk, min((s+1)*chunk, lens[b])) of KV head g and the G query rows of
// that group, as k_attn_decode (decode.hip).  A lane holds E consecutive
// bytes of a key (E = 16: one 16-byte load; E = 8 at G = 8), so D/E adjacent
// lanes are one key group, the block has 256/(D/E) of them, and key group j
// takes the keys tile + j, tile + j + groups, ... of each 128-key tile: the
// loads of one instruction of a wave are consecutive keys, 1 KB (E = 16) or
// 512 B contiguous.  Per tile a lane issues all its K and V loads, then per
// key: packed converts to fp32, the partial dot product with every query row
// and a butterfly sum over the key group; then ONE online-softmax update per
// query row for the tile's keys (the scores turn into probabilities in
// place), and per key one unpack of V shared by all query rows.  Each key
// group keeps its own (m, l, o) per query row; the key groups of a wave merge
// by shuffles, the four waves through LDS in wave order.  Keys at or past the
// end of the range are neither loaded nor used.
//
// Outputs as k_attn_decode: part_ml [B][H][n_splits][2], part_o
// [B][H][n_splits][D] fp32 (v_scale applied), or with o_direct (n_splits ==
// 1) bf16 O[b][h*D + d]; an empty range writes m = -inf, l = 0, o = 0.
template <int E>
struct Raw {
  uint32_t w[E / 4];
};

template <int E>
__device__ __forceinline__ Raw<E> load_raw(const uint8_t* p) {
  Raw<E> r;
  if constexpr (E == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    r.w[0] = v.x, r.w[1] = v.y, r.w[2] = v.z, r.w[3] = v.w;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    r.w[0] = v.x, r.w[1] = v.y;
  }
  return r;
}

template <int E>
__device__ __forceinline__ void unpack_raw(const Raw<E>& r, float* v) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i) unpack4(r.w[i], v + 4 * i);
}

template <int D, int G, int E>
__global__ __launch_bounds__(NT) void k_attn_decode_fp8(const uint16_t* __restrict__ q, long long q_stride,
                                                        const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                        const float* __restrict__ kv_scale,
                                                        const int* __restrict__ lens, float* __restrict__ part_ml,
                                                        float* __restrict__ part_o, uint16_t* __restrict__ o_direct,
                                                        long long o_stride, int H, int Hkv, int max_len, int chunk,
                                                        float qk_scale) {
  constexpr int LPK = D / E;      // lanes per key
  constexpr int NGRP = NT / LPK;  // key groups per block
  constexpr int U = KT8 / NGRP;   // keys per key group per tile
  __shared__ float sm[4][G][D + 2];
  const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int nsplit = gridDim.x;
  const int tid = threadIdx.x, sub = tid % LPK, grp = tid / LPK;
  const int h0 = g * G;
  int len = lens[b];
  len = len < 0 ? 0 : (len > max_len ? max_len : len);
  const int lo = s * chunk;
  const int hi = (lo + chunk < len) ? lo + chunk : len;
  if (hi <= lo) {  // uniform over the block: no barrier below is skipped by a part of it
    for (int i = tid; i < G * D; i += NT) {
      const int gq = i / D, d = i % D;
      if (o_direct)
        o_direct[(long long)b * o_stride + (long long)(h0 + gq) * D + d] = 0;
      else
        part_o[(((long long)b * H + h0 + gq) * nsplit + s) * D + d] = 0.f;
    }
    if (!o_direct && tid < G) {
      float* ml = part_ml + (((long long)b * H + h0 + tid) * nsplit + s) * 2;
      ml[0] = -INFINITY;
      ml[1] = 0.f;
    }
    return;
  }

  const float qs = qk_scale * kv_scale[g];  // k_scale * D^-0.5 * log2e
  const float v_scale = kv_scale[Hkv + g];
  float qf[G][E];
#pragma unroll
  for (int gq = 0; gq < G; ++gq) {
    const uint16_t* qp = q + (long long)b * q_stride + (long long)(h0 + gq) * D + sub * E;
#pragma unroll
    for (int c = 0; c < E / 8; ++c) {
      uint16_t x[8];
      split8(*reinterpret_cast<const uint4*>(qp + c * 8), x);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[gq][c * 8 + e] = bf2f(x[e]) * qs;
    }
  }
  float m[G], l[G], acc[G][E];
#pragma unroll
  for (int gq = 0; gq < G; ++gq) {
    m[gq] = -INFINITY;
    l[gq] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[gq][e] = 0.f;
  }
  const long long head_off = ((long long)b * Hkv + g) * max_len * D + sub * E;
  const uint8_t* kb = kc + head_off;
  const uint8_t* vb = vc + head_off;

  for (int base = lo; base < hi; base += KT8) {
    Raw<E> kr[U], vr[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * NGRP + grp;
      ok[u] = key < hi;
      kr[u] = ok[u] ? load_raw<E>(kb + (long long)key * D) : Raw<E>{};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * NGRP + grp;
      vr[u] = ok[u] ? load_raw<E>(vb + (long long)key * D) : Raw<E>{};
    }
    float sc[U][G];  // scores, then probabilities
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[E];
      unpack_raw<E>(kr[u], kf);
#pragma unroll
      for (int gq = 0; gq < G; ++gq) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) d += qf[gq][e] * kf[e];
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        sc[u][gq] = ok[u] ? d : -INFINITY;
      }
    }
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
      float mn = m[gq];
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[u][gq]);
      const float ms = (mn == -INFINITY) ? 0.f : mn;  // a key group with no key yet: everything stays 0
      const float alpha = exp2f(m[gq] - ms);
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sc[u][gq] = exp2f(sc[u][gq] - ms);
        ps += sc[u][gq];
      }
      l[gq] = l[gq] * alpha + ps;
      m[gq] = mn;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[gq][e] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[E];
      unpack_raw<E>(vr[u], vf);
#pragma unroll
      for (int gq = 0; gq < G; ++gq)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[gq][e] += sc[u][gq] * vf[e];
    }
  }

  // the key groups of a wave -> its lanes 0..LPK-1
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
      const float mo = __shfl_xor(m[gq], off, 64), lo2 = __shfl_xor(l[gq], off, 64);
      const float mn = fmaxf(m[gq], mo);
      const float ms = (mn == -INFINITY) ? 0.f : mn;
      const float a = exp2f(m[gq] - ms), c = exp2f(mo - ms);
      l[gq] = l[gq] * a + lo2 * c;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[gq][e] = acc[gq][e] * a + __shfl_xor(acc[gq][e], off, 64) * c;
      m[gq] = mn;
    }
  }
  const int w = tid >> 6;
  if ((tid & 63) < LPK) {
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
#pragma unroll
      for (int e = 0; e < E; ++e) sm[w][gq][sub * E + e] = acc[gq][e];
      if (sub == 0) {
        sm[w][gq][D] = m[gq];
        sm[w][gq][D + 1] = l[gq];
      }
    }
  }
  __syncthreads();
  // the four waves, in wave order; v_scale once, on the merged accumulator
  for (int i = tid; i < G * D; i += NT) {
    const int gq = i / D, d = i % D;
    float M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, sm[ww][gq][D]);
    const float ms = (M == -INFINITY) ? 0.f : M;
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float c = exp2f(sm[ww][gq][D] - ms);
      L += sm[ww][gq][D + 1] * c;
      O += sm[ww][gq][d] * c;
    }
    O *= v_scale;
    if (o_direct) {
      o_direct[(long long)b * o_stride + (long long)(h0 + gq) * D + d] = f2bf(L > 0.f ? O / L : 0.f);
    } else {
      const long long r = ((long long)b * H + h0 + gq) * nsplit + s;
      part_o[r * D + d] = O;
      if (d == 0) {
        part_ml[r * 2] = M;
        part_ml[r * 2 + 1] = L;
      }
    }
  }
}

// Grid (H, B), 128 threads, thread d folds the n_splits partials of (b, h) in
// split order: decode.hip's combine (private to that file) on the same
// partial layout.  A head with no key at all gives zeros.
__global__ __launch_bounds__(128) void k_attn_decode_fp8_combine(const float* __restrict__ part_ml,
                                                                 const float* __restrict__ part_o,
                                                                 uint16_t* __restrict__ o, long long o_stride, int H,
                                                                 int D, int nsplit) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  if (d >= D) return;
  const long long r0 = ((long long)b * H + h) * nsplit;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, part_ml[(r0 + s) * 2]);
  const float ms = (M == -INFINITY) ? 0.f : M;
  float L = 0.f, O = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float c = exp2f(part_ml[(r0 + s) * 2] - ms);
    L += part_ml[(r0 + s) * 2 + 1] * c;
    O += part_o[(r0 + s) * D + d] * c;
  }
  o[(long long)b * o_stride + (long long)h * D + d] = f2bf(L > 0.f ? O / L : 0.f);
}

template <int D>
int launch_decode_fp8(int G, dim3 grid, hipStream_t s, const uint16_t* q, long long q_stride, const uint8_t* kc,
                      const uint8_t* vc, const float* kv_scale, const int* lens, float* part_ml, float* part_o,
                      uint16_t* o_direct, long long o_stride, int H, int Hkv, int max_len, int chunk, float qk_scale) {
#define PTO_DECODE_FP8_CASE(GG, EE)                                                                                \
  case GG:                                                                                                         \
    hipLaunchKernelGGL((k_attn_decode_fp8<D, GG, EE>), grid, dim3(NT), 0, s, q, q_stride, kc, vc, kv_scale, lens,  \
                       part_ml, part_o, o_direct, o_stride, H, Hkv, max_len, chunk, qk_scale);                     \
    break;
  switch (G) {
    PTO_DECODE_FP8_CASE(1, 16)
    PTO_DECODE_FP8_CASE(2, 16)
    PTO_DECODE_FP8_CASE(4, 16)
    PTO_DECODE_FP8_CASE(8, 8)
    default:
      return -1;
  }
#undef PTO_DECODE_FP8_CASE
  return 0;
}

}  // namespace

#define PTO_API extern "C" __attribute__((visibility("default")))

// qkv [B*T][(H + 2*Hkv)*D] bf16 contiguous, cs/sn fp32 [table_len][D/2],
// k_cache/v_cache e4m3 [B][Hkv][max_len][D], kv_scale fp32 [4][Hkv], lens
// int32 [B], n_new int32 [B] or null (all T tokens of every row count).
PTO_API int pto_rope_kv_extend_fp8(void* qkv, const float* cs, const float* sn, void* k_cache, void* v_cache,
                                   const float* kv_scale, const int* lens, const int* n_new, int B, int T, int H,
                                   int Hkv, int D, int max_len, int table_len, hipStream_t s) {
  if (D % 16 || B < 0 || T < 0 || H < 1 || Hkv < 1 || max_len < 1 || table_len < 1 || !kv_scale) return -1;
  if (((((uintptr_t)qkv) | ((uintptr_t)cs) | ((uintptr_t)sn)) & 15) ||
      ((((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 7))
    return -1;
  if (B == 0 || T == 0) return 0;
  long long blocks = ((long long)B * T * (H + 2 * Hkv) * (D / 16) + NT - 1) / NT;
  if (blocks > 65535) blocks = 65535;
  hipLaunchKernelGGL(k_rope_kv_extend_fp8, dim3((unsigned)blocks), dim3(NT), 0, s, (uint16_t*)qkv, cs, sn,
                     (uint8_t*)k_cache, (uint8_t*)v_cache, kv_scale, lens, n_new, B, T, H, Hkv, D, max_len, table_len,
                     1.f);
  return (int)hipGetLastError();
}

// Keys per split: fixed by max_len and n_splits alone, a multiple of the 128-key tile.
PTO_API int pto_attn_decode_fp8_chunk(int max_len, int n_splits) {
  if (max_len < 1 || n_splits < 1) return -1;
  const int c = (max_len + n_splits - 1) / n_splits;
  return (c + KT8 - 1) / KT8 * KT8;
}

// pto_attn_decode (decode.hip) on e4m3 caches: q bf16 at q + b*q_stride + h*D,
// o bf16 [B][H*D], part_ml / part_o fp32 workspaces of B*H*n_splits*2 and
// B*H*n_splits*D floats (unused when n_splits == 1).
PTO_API int pto_attn_decode_fp8(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                const float* kv_scale, const int* lens, void* o, float* part_ml, float* part_o, int B,
                                int H, int Hkv, int D, int max_len, int n_splits, float scale, hipStream_t s) {
  if (H < 1 || Hkv < 1 || H % Hkv || (D != 64 && D != 128) || !kv_scale) return -1;
  const int G = H / Hkv;
  if ((G != 1 && G != 2 && G != 4 && G != 8) || max_len < 1 || n_splits < 1 || n_splits > 65535 || Hkv > 65535 ||
      B > 65535 || (q_stride % 8) || ((((uintptr_t)q) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15))
    return -1;
  if (B <= 0) return 0;
  if (n_splits > 1 && (!part_ml || !part_o)) return -1;
  const int chunk = pto_attn_decode_fp8_chunk(max_len, n_splits);
  const float qk_scale = scale * 1.4426950408889634f;
  uint16_t* od = n_splits == 1 ? (uint16_t*)o : nullptr;
  const dim3 grid(n_splits, Hkv, B);
  const long long o_stride = (long long)H * D;
  int rc;
  if (D == 128)
    rc = launch_decode_fp8<128>(G, grid, s, (const uint16_t*)q, q_stride, (const uint8_t*)k_cache,
                                (const uint8_t*)v_cache, kv_scale, lens, part_ml, part_o, od, o_stride, H, Hkv,
                                max_len, chunk, qk_scale);
  else
    rc = launch_decode_fp8<64>(G, grid, s, (const uint16_t*)q, q_stride, (const uint8_t*)k_cache,
                               (const uint8_t*)v_cache, kv_scale, lens, part_ml, part_o, od, o_stride, H, Hkv, max_len,
                               chunk, qk_scale);
  if (rc) return rc;
  if (n_splits > 1)
    hipLaunchKernelGGL(k_attn_decode_fp8_combine, dim3(H, B), dim3(128), 0, s, part_ml, part_o, (uint16_t*)o, o_stride,
                       H, D, n_splits);
  return (int)hipGetLastError();
}
