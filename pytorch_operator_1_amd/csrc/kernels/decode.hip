// KV-cache generation kernels of the Llama model (models/llama.py
// Llama.decode_step / generate): everything one decode step needs besides
// the GEMMs and the kernels of llm_kernels.hip it shares with training.
//
//   rope_kv_append   rotate the new row's query heads in place, write its
//                    rotated K head and its V head into the caches at lens[b]
//   attn_decode      one query row per head against the cached history,
//                    split over the history (split-KV) + an ordered combine
//   sample           greedy / temperature / top-k token choice on bf16
//                    logits, with the step bookkeeping (cur, out, done)
//   decode_advance   step[0] += 1, lens[b] += 1
//
// Everything is device-driven: the current length of every batch row is the
// device int32 lens[B] and no launch parameter depends on it, so one decode
// step captures into a HIP graph once and replays for every token.
//
// Caches are bf16 [B][Hkv][max_len][D]: one head's keys are contiguous.
//
// attn_decode uses VALU dot products, not MFMA.  The kernel reads every K/V
// byte once and does 4*G FLOP per byte pair (about 4 FLOP/B at G = 4), far
// below the machine balance, so the matrix cores have nothing to win; an
// MFMA tile would need 16 or 32 query rows to be full and decode has G <= 8,
// and it would need the K tile transposed through LDS.  With VALU FMAs each
// lane keeps the 8 elements of its 16-byte load, K/V go straight from global
// memory to VGPRs and the main loop has no LDS traffic and no barrier.
//
// Determinism: no atomics on floats anywhere.  The bits of O depend only on
// (inputs, lens, max_len, n_splits): each block folds its keys in a fixed
// order, the combine folds the splits in split order.  sample is a
// deterministic function of (logits, u, temperature, top_k).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ void unpack8(const uint4 q, float* v) {  // bf16x8 -> 8 floats
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

constexpr int NT = 256;

// ---------------------------------------------------------------- rope_kv_append
// qkv row b = [H q heads | Hkv k heads | Hkv v heads] x D of the new token of
// batch row b, p = lens[b] its position.  The arithmetic is k_rope's
// (llm_kernels.hip), expression for expression, 4 rotate_half pairs (i,
// i + D/2) per thread: a key appended at p is bitwise the key rope_ produces
// for the same row at position p.  q heads are rotated in place, the rotated
// k head goes to k_cache[b][g][p], the v head is copied to v_cache[b][g][p].
// A row with p outside [0, min(max_len, table_len)) writes nothing at all.
__global__ __launch_bounds__(NT) void k_rope_kv_append(uint16_t* qkv, const float* __restrict__ cs,
                                                       const float* __restrict__ sn, uint16_t* __restrict__ kc,
                                                       uint16_t* __restrict__ vc, const int* __restrict__ lens, int B,
                                                       int H, int Hkv, int D, int max_len, int table_len, float sign) {
  const int H2 = D >> 1, Q = H2 >> 2;
  const int nh = H + 2 * Hkv;
  const long long total = (long long)B * nh * Q;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int q = (int)(i % Q);
    const long long t = i / Q;
    const int hd = (int)(t % nh);
    const int b = (int)(t / nh);
    const int p = lens[b];
    if (p < 0 || p >= max_len || p >= table_len) continue;
    const long long off = (long long)b * nh * D + (long long)hd * D + q * 4;
    const uint2 lo = *reinterpret_cast<const uint2*>(qkv + off), hi = *reinterpret_cast<const uint2*>(qkv + off + H2);
    if (hd >= H + Hkv) {  // v head: a copy
      uint16_t* base = vc + (((long long)b * Hkv + (hd - H - Hkv)) * max_len + p) * D + q * 4;
      *reinterpret_cast<uint2*>(base) = lo;
      *reinterpret_cast<uint2*>(base + H2) = hi;
      continue;
    }
    uint16_t* base = hd < H ? qkv + off : kc + (((long long)b * Hkv + (hd - H)) * max_len + p) * D + q * 4;
    const float4 c = *reinterpret_cast<const float4*>(cs + (long long)p * H2 + q * 4);
    const float4 n = *reinterpret_cast<const float4*>(sn + (long long)p * H2 + q * 4);
    const float x1[4] = {__uint_as_float(lo.x << 16), __uint_as_float(lo.x & 0xffff0000u), __uint_as_float(lo.y << 16),
                         __uint_as_float(lo.y & 0xffff0000u)};
    const float x2[4] = {__uint_as_float(hi.x << 16), __uint_as_float(hi.x & 0xffff0000u), __uint_as_float(hi.y << 16),
                         __uint_as_float(hi.y & 0xffff0000u)};
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sign * n.x, sign * n.y, sign * n.z, sign * n.w};
    uint16_t o1[4], o2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o1[e] = f2bf(x1[e] * cc[e] - x2[e] * ss[e]);
      o2[e] = f2bf(x2[e] * cc[e] + x1[e] * ss[e]);
    }
    *reinterpret_cast<uint2*>(base) = uint2{(uint32_t)o1[0] | ((uint32_t)o1[1] << 16), (uint32_t)o1[2] | ((uint32_t)o1[3] << 16)};
    *reinterpret_cast<uint2*>(base + H2) =
        uint2{(uint32_t)o2[0] | ((uint32_t)o2[1] << 16), (uint32_t)o2[2] | ((uint32_t)o2[3] << 16)};
  }
}

// ---------------------------------------------------------------- attn_decode
// Grid (n_splits, Hkv, B), 256 threads.  Block (s, g, b) owns the keys
// [s*chunk, min((s+1)*chunk, lens[b])) of KV head g and the G = H/Hkv query
// rows of that group.  A key row of D bf16 is D/8 16-byte loads, so D/8
// adjacent lanes (a "key group": 16 lanes at D = 128, 8 at D = 64) hold one
// key; the block has 256/(D/8) key groups and walks its range in tiles of
// KT = 64 keys, key group j taking the keys tile + j, tile + j + groups, ...
// (a wave's loads of one instruction are consecutive keys: 1 KB contiguous).
// Per tile a lane issues all its K and V loads, then for every query row:
// 8 FMAs per key, a butterfly sum over the key group, and ONE online-softmax
// update (fp32, exp2 form: q is pre-multiplied by scale*log2e) for the
// tile's keys.  Each key group keeps its own (m, l, o) per query row; at the
// end the key groups of a wave merge by shuffles, the four waves through
// LDS, in wave order.  Keys at or past the end of the range are neither
// loaded nor used (the cache tail may hold anything).
//
// part_ml [B][H][n_splits][2] = (m, l), part_o [B][H][n_splits][D] fp32; a
// block with an empty range writes m = -inf, l = 0, o = 0 and leaves as a
// whole (the test is uniform over the block).  o_direct != nullptr
// (n_splits == 1): write bf16 O[b][h*D + d] = o / l instead (zeros for an
// empty history).
constexpr int KT = 64;

template <int D, int G>
__global__ __launch_bounds__(NT) void k_attn_decode(const uint16_t* __restrict__ q, long long q_stride,
                                                    const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                    const int* __restrict__ lens, float* __restrict__ part_ml,
                                                    float* __restrict__ part_o, uint16_t* __restrict__ o_direct,
                                                    long long o_stride, int H, int Hkv, int max_len, int chunk,
                                                    float qk_scale) {
  constexpr int LPK = D / 8;      // lanes per key
  constexpr int NGRP = NT / LPK;  // key groups per block
  constexpr int U = KT / NGRP;    // keys per key group per tile
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

  float qf[G][8];
#pragma unroll
  for (int gq = 0; gq < G; ++gq) {
    unpack8(*reinterpret_cast<const uint4*>(q + (long long)b * q_stride + (long long)(h0 + gq) * D + sub * 8), qf[gq]);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[gq][e] *= qk_scale;
  }
  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int gq = 0; gq < G; ++gq) {
    m[gq] = -INFINITY;
    l[gq] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[gq][e] = 0.f;
  }
  const long long head_off = ((long long)b * Hkv + g) * max_len * D + sub * 8;
  const uint16_t* kb = kc + head_off;
  const uint16_t* vb = vc + head_off;

  for (int base = lo; base < hi; base += KT) {
    uint4 kr[U], vr[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * NGRP + grp;
      ok[u] = key < hi;
      kr[u] = ok[u] ? *reinterpret_cast<const uint4*>(kb + (long long)key * D) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * NGRP + grp;
      vr[u] = ok[u] ? *reinterpret_cast<const uint4*>(vb + (long long)key * D) : uint4{0, 0, 0, 0};
    }
    float sc[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
#pragma unroll
      for (int gq = 0; gq < G; ++gq) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d += qf[gq][e] * kf[e];
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        sc[u][gq] = ok[u] ? d : -INFINITY;
      }
    }
    float vf[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) unpack8(vr[u], vf[u]);
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
      float mn = m[gq];
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[u][gq]);
      const float ms = (mn == -INFINITY) ? 0.f : mn;  // a key group with no key yet: everything stays 0
      const float alpha = exp2f(m[gq] - ms);
      float p[U], ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        p[u] = exp2f(sc[u][gq] - ms);
        ps += p[u];
      }
      l[gq] = l[gq] * alpha + ps;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = acc[gq][e] * alpha;
#pragma unroll
        for (int u = 0; u < U; ++u) a += p[u] * vf[u][e];
        acc[gq][e] = a;
      }
      m[gq] = mn;
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
      for (int e = 0; e < 8; ++e) acc[gq][e] = acc[gq][e] * a + __shfl_xor(acc[gq][e], off, 64) * c;
      m[gq] = mn;
    }
  }
  const int w = tid >> 6;
  if ((tid & 63) < LPK) {
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[w][gq][sub * 8 + e] = acc[gq][e];
      if (sub == 0) {
        sm[w][gq][D] = m[gq];
        sm[w][gq][D + 1] = l[gq];
      }
    }
  }
  __syncthreads();
  // the four waves, in wave order
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

// Grid (H, B), 128 threads, thread d folds the n_splits partials of (b, h)
// in split order.  A head with no key at all (lens[b] == 0) gives zeros.
__global__ __launch_bounds__(128) void k_attn_decode_combine(const float* __restrict__ part_ml,
                                                             const float* __restrict__ part_o,
                                                             uint16_t* __restrict__ o, long long o_stride, int H, int D,
                                                             int nsplit) {
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

// ---------------------------------------------------------------- sample
// One block per row of V bf16 logits, V % 8 == 0 (the launcher refuses
// anything else, as k_ce_eval's does: no scalar tail).
//   greedy (temperature <= 0): argmax, the lowest index among equal maxima
//     (torch.argmax's rule; float compares, so -0 == +0).
//   top_k in (0, V): the k-th largest value thr is found exactly by two
//     256-bin radix passes over the order-preserving 16-bit keys of the row
//     (integer LDS histograms); kept = {i : z[i] >= thr}, ties included.
//   sampling: w[i] = exp((z[i] - max) / temperature) on the kept set.  Thread
//     t owns the contiguous indices [t*span, (t+1)*span) and sums its w in
//     index order; thread 0 scans the 256 sums in thread order.  With
//     cdf[i] = prefix[t] + (thread t's running sum up to and including i),
//     the token is the first kept i with cdf[i] > u * total; if rounding
//     leaves none, the last kept index.
// Bookkeeping: st = step[0] (0 without step); a row whose done[b] is set
// emits eos_id; the token goes to cur[b] and to out[b][st] (st < n_steps);
// a row that emits eos_id (>= 0) sets done[b].  u is [n_steps][B].
__device__ __forceinline__ uint32_t okey(uint32_t bits) {  // bf16 bits -> key, larger float = larger key
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}
__device__ __forceinline__ float key2f(uint32_t key) {
  const uint32_t bits = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(bits << 16);
}

__global__ __launch_bounds__(NT) void k_sample(const uint16_t* __restrict__ logits, const float* __restrict__ u,
                                               long long* __restrict__ cur, long long* __restrict__ out, int n_steps,
                                               const int* __restrict__ step, int* __restrict__ done, int V, int B,
                                               float temperature, int top_k, long long eos_id) {
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ int hist[256];
  __shared__ float pref[NT + 1];
  __shared__ int sel[2];
  __shared__ int pick[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int st = step ? step[0] : 0;
  if (done && done[b] != 0) {  // the whole block leaves
    if (tid == 0) {
      if (cur) cur[b] = eos_id;
      if (out && st >= 0 && st < n_steps) out[(long long)b * n_steps + st] = eos_id;
    }
    return;
  }
  const uint16_t* z = logits + (long long)b * V;
  const int n8 = V >> 3;

  // maximum and its first index
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int i = tid; i < n8; i += NT) {
    float a[8];
    unpack8(*reinterpret_cast<const uint4*>(z + i * 8), a);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (a[e] > bv) {
        bv = a[e];
        bi = i * 8 + e;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    redf[tid >> 6] = bv;
    redi[tid >> 6] = bi;
  }
  if (tid == 0) {
    pick[0] = INT_MAX;
    pick[1] = -1;
  }
  __syncthreads();
  float gmax = redf[0];
  int gidx = redi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (redf[w] > gmax || (redf[w] == gmax && redi[w] < gidx)) {
      gmax = redf[w];
      gidx = redi[w];
    }
  if (gidx == INT_MAX) gidx = 0;  // nothing above -inf
  int tok = gidx;

  if (temperature > 0.f) {  // uniform over the block
    float thr = -INFINITY;
    if (top_k > 0 && top_k < V) {
      for (int pass = 0; pass < 2; ++pass) {
        hist[tid] = 0;
        __syncthreads();
        const uint32_t hi_sel = pass ? (uint32_t)sel[0] : 0u;
        for (int i = tid; i < n8; i += NT) {
          const uint4 qv = *reinterpret_cast<const uint4*>(z + i * 8);
          const uint32_t wv[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const uint32_t key = okey((wv[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            if (pass == 0)
              atomicAdd(&hist[key >> 8], 1);
            else if ((key >> 8) == hi_sel)
              atomicAdd(&hist[key & 255u], 1);
          }
        }
        __syncthreads();
        if (tid == 0) {
          int cum = pass ? sel[1] : 0, bin = 0;
          for (int c = 255; c >= 0; --c) {
            if (cum + hist[c] >= top_k) {
              bin = c;
              break;
            }
            cum += hist[c];
          }
          if (pass == 0) {
            sel[0] = bin;
            sel[1] = cum;  // keys in higher bins
          } else {
            sel[1] = bin;
          }
        }
        __syncthreads();
      }
      thr = key2f(((uint32_t)sel[0] << 8) | (uint32_t)sel[1]);
    }
    const float inv_t = 1.f / temperature;
    const int span = (n8 + NT - 1) / NT;
    const int c0 = tid * span < n8 ? tid * span : n8;
    const int c1 = c0 + span < n8 ? c0 + span : n8;
    float local = 0.f;
    int last = -1;
    for (int i = c0; i < c1; ++i) {
      float a[8];
      unpack8(*reinterpret_cast<const uint4*>(z + i * 8), a);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (a[e] >= thr) {
          local += __expf((a[e] - gmax) * inv_t);
          last = i * 8 + e;
        }
    }
    pref[tid + 1] = local;
    if (last >= 0) atomicMax(&pick[1], last);
    __syncthreads();
    if (tid == 0) {
      float run = 0.f;
      for (int t = 0; t < NT; ++t) {
        const float v = pref[t + 1];
        pref[t] = run;  // exclusive prefix of thread t
        run += v;
      }
      pref[NT] = run;
    }
    __syncthreads();
    const int su = (st < 0) ? 0 : (st < n_steps ? st : n_steps - 1);
    const float target = u[(long long)su * B + b] * pref[NT];
    const float pre = pref[tid];
    if (pre <= target && target < pref[tid + 1]) {
      float run = 0.f;
      int found = INT_MAX;
      for (int i = c0; i < c1 && found == INT_MAX; ++i) {
        float a[8];
        unpack8(*reinterpret_cast<const uint4*>(z + i * 8), a);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (a[e] >= thr) {
            run += __expf((a[e] - gmax) * inv_t);
            if (found == INT_MAX && pre + run > target) found = i * 8 + e;
          }
      }
      if (found != INT_MAX) atomicMin(&pick[0], found);
    }
    __syncthreads();
    tok = pick[0] != INT_MAX ? pick[0] : (pick[1] >= 0 ? pick[1] : gidx);
  }

  if (tid == 0) {
    if (cur) cur[b] = tok;
    if (out && st >= 0 && st < n_steps) out[(long long)b * n_steps + st] = tok;
    if (done && eos_id >= 0 && (long long)tok == eos_id) done[b] = 1;
  }
}

// step[0] += 1 and lens[b] += 1 after a token has been chosen (a launch of
// its own: every k_sample block has read step[0] by then).
__global__ __launch_bounds__(NT) void k_decode_advance(int* __restrict__ step, int* __restrict__ lens, int B) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < B && lens) lens[i] += 1;
  if (i == 0 && step) step[0] += 1;
}

inline unsigned grid_for(long long items) {
  long long g = (items + NT - 1) / NT;
  if (g < 1) g = 1;
  if (g > 65535) g = 65535;
  return (unsigned)g;
}

}  // namespace

#define PTO_API extern "C" __attribute__((visibility("default")))

// qkv [B][(H + 2*Hkv)*D] bf16 contiguous, cs/sn fp32 [table_len][D/2],
// k_cache/v_cache bf16 [B][Hkv][max_len][D], lens int32 [B].
PTO_API int pto_rope_kv_append(void* qkv, const float* cs, const float* sn, void* k_cache, void* v_cache,
                               const int* lens, int B, int H, int Hkv, int D, int max_len, int table_len,
                               hipStream_t s) {
  if (D % 8 || B < 0 || H < 1 || Hkv < 1 || max_len < 1 || table_len < 1) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_rope_kv_append, dim3(grid_for((long long)B * (H + 2 * Hkv) * (D / 8))), dim3(NT), 0, s,
                     (uint16_t*)qkv, cs, sn, (uint16_t*)k_cache, (uint16_t*)v_cache, lens, B, H, Hkv, D, max_len,
                     table_len, 1.f);
  return (int)hipGetLastError();
}

PTO_API int pto_attn_decode_supported(int H, int Hkv, int D) {
  if (H < 1 || Hkv < 1 || H % Hkv) return 0;
  const int G = H / Hkv;
  return (D == 64 || D == 128) && (G == 1 || G == 2 || G == 4 || G == 8);
}

// Keys per split: fixed by max_len and n_splits alone, a multiple of the key tile.
PTO_API int pto_attn_decode_chunk(int max_len, int n_splits) {
  if (max_len < 1 || n_splits < 1) return -1;
  const int c = (max_len + n_splits - 1) / n_splits;
  return (c + KT - 1) / KT * KT;
}

template <int D>
static int launch_decode(int G, dim3 grid, hipStream_t s, const uint16_t* q, long long q_stride, const uint16_t* kc,
                         const uint16_t* vc, const int* lens, float* part_ml, float* part_o, uint16_t* o_direct,
                         long long o_stride, int H, int Hkv, int max_len, int chunk, float qk_scale) {
#define PTO_DECODE_CASE(GG)                                                                                        \
  case GG:                                                                                                         \
    hipLaunchKernelGGL((k_attn_decode<D, GG>), grid, dim3(NT), 0, s, q, q_stride, kc, vc, lens, part_ml, part_o,   \
                       o_direct, o_stride, H, Hkv, max_len, chunk, qk_scale);                                      \
    break;
  switch (G) {
    PTO_DECODE_CASE(1)
    PTO_DECODE_CASE(2)
    PTO_DECODE_CASE(4)
    PTO_DECODE_CASE(8)
    default:
      return -1;
  }
#undef PTO_DECODE_CASE
  return 0;
}

// q: the new rows' query heads, bf16, head h of batch row b at q + b*q_stride
// + h*D (elements); o bf16 [B][H*D].  part_ml / part_o: fp32 workspaces of
// B*H*n_splits*2 and B*H*n_splits*D floats (unused when n_splits == 1).
PTO_API int pto_attn_decode(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                            const int* lens, void* o, float* part_ml, float* part_o, int B, int H, int Hkv, int D,
                            int max_len, int n_splits, float scale, hipStream_t s) {
  if (!pto_attn_decode_supported(H, Hkv, D) || max_len < 1 || n_splits < 1 || n_splits > 65535 || Hkv > 65535 ||
      B > 65535 || (q_stride % 8) || ((((uintptr_t)q) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15))
    return -1;
  if (B <= 0) return 0;
  if (n_splits > 1 && (!part_ml || !part_o)) return -1;
  const int chunk = pto_attn_decode_chunk(max_len, n_splits);
  const float qk_scale = scale * 1.4426950408889634f;
  uint16_t* od = n_splits == 1 ? (uint16_t*)o : nullptr;
  const dim3 grid(n_splits, Hkv, B);
  const int G = H / Hkv;
  const long long o_stride = (long long)H * D;
  int rc;
  if (D == 128)
    rc = launch_decode<128>(G, grid, s, (const uint16_t*)q, q_stride, (const uint16_t*)k_cache,
                            (const uint16_t*)v_cache, lens, part_ml, part_o, od, o_stride, H, Hkv, max_len, chunk,
                            qk_scale);
  else
    rc = launch_decode<64>(G, grid, s, (const uint16_t*)q, q_stride, (const uint16_t*)k_cache,
                           (const uint16_t*)v_cache, lens, part_ml, part_o, od, o_stride, H, Hkv, max_len, chunk,
                           qk_scale);
  if (rc) return rc;
  if (n_splits > 1)
    hipLaunchKernelGGL(k_attn_decode_combine, dim3(H, B), dim3(128), 0, s, part_ml, part_o, (uint16_t*)o, o_stride, H,
                       D, n_splits);
  return (int)hipGetLastError();
}

// logits bf16 [B][V] (16-byte aligned, V % 8 == 0), u fp32 [n_steps][B] (may
// be null when temperature <= 0), cur int64 [B], out int64 [B][n_steps],
// step int32 [1], done int32 [B] (cur, out, step, done may be null).
// advance != 0: also step[0] += 1 and lens[b] += 1 (lens may be null).
PTO_API int pto_sample(const void* logits, const float* u, long long* cur, long long* out, int n_steps,
                       int* step, int* done, int B, int V, float temperature, int top_k, long long eos_id,
                       int advance, int* lens, hipStream_t s) {
  if (V < 8 || V % 8 || n_steps < 1 || (((uintptr_t)logits) & 15)) return -1;
  if (temperature > 0.f && !u) return -1;
  if (!(temperature >= 0.f)) return -1;
  if (B <= 0) return 0;
  hipLaunchKernelGGL(k_sample, dim3((unsigned)B), dim3(NT), 0, s, (const uint16_t*)logits, u, cur, out, n_steps, step,
                     done, V, B, temperature, top_k, eos_id);
  if (advance)
    hipLaunchKernelGGL(k_decode_advance, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, s, step, lens, B);
  return (int)hipGetLastError();
}
