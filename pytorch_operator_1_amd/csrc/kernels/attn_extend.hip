// Multi-token extend on the KV cache (models/llama.py Llama.extend, chunked
// Llama.prefill): T new tokens per batch row against the cached history.
//
//   rope_kv_extend   rotate the query heads of the T new rows in place, write
//                    their rotated K heads and their V heads into the caches
//                    at lens[b] + t
//   attn_extend      T*G query rows per KV head against the cache, on
//                    v_mfma_f32_32x32x16_bf16, split over the history, and an
//                    ordered combine of the splits
//
// Token t of row b is LIVE iff 0 <= t < n_new[b] and 0 <= lens[b] + t < limit
// (limit = min(max_len, table_len) for the append, max_len for the attention).
// lens is the device int32 [B] length BEFORE the append, n_new the device
// int32 [B] count of real tokens of a right-padded chunk.  No launch parameter
// depends on either, so both launches capture into a graph.
//
// Why a kernel of its own next to k_attn_decode (decode.hip): there one query
// row per head cannot fill a matrix tile, so VALU dot products are right.
// Here the T*G query rows that share one KV head fill a 32-row MFMA tile from
// T = 8 at G = 4 on, and the K/V bytes are read once for all T tokens.
//
// attn_extend, grid (n_splits, Hkv, B * row_tiles), 256 threads:
//   * Query row r = t*G + gq of KV head g; a block owns the 32-row tile
//     [32*rt, 32*rt + 32) (G divides 32: a token's heads never straddle a
//     tile) and the keys [s*chunk, min((s+1)*chunk, end)), end = lens[b] +
//     (live tokens up to the tile's last one).  chunk is a function of
//     (max_len, n_splits) alone.  Row r attends to keys [0, lens[b] + t + 1).
//   * Swapped products as in k_attn_fwd (attention.hip): S^T = K Q^T and
//     O^T = V^T P^T, the query on the lane, so the online softmax is
//     lane-local plus one cross-half exchange and the rescale is a per-lane
//     scalar.  The Q fragments (B operand) are loaded once and stay in VGPRs;
//     the scale is applied to the fp32 scores (p = exp2(s*c - m), one fma), not
//     to the bf16 Q, which would round it a second time.
//   * The four waves take interleaved 32-key slabs (wave w: lo + 32*w + 128*i),
//     each with its own (m, l, O^T).  K never touches LDS: a key row is D
//     contiguous bf16, so lane l loading the 16 bytes of key slab + (l & 31) at
//     chunk 2*ks + (l >> 5) already holds the A operand of k-step ks.  V goes
//     through a wave-PRIVATE swizzled LDS slab (32 keys x D) and comes back
//     transposed with ds_read_b64_tr_b16, so the main loop has no block-wide
//     barrier.  The next slab's V loads are issued before this slab's MFMAs,
//     its K loads right after the S^T MFMAs have consumed this slab's K
//     registers (236 VGPRs at D = 128: two waves per SIMD, nothing spilled).
//     P^T's B operand is built from the accumulator with v_cvt_pk_bf16_f32 +
//     v_permlane32_swap.
//   * Masking.  Nothing the cache holds at or past the block's end (so nothing
//     past lens[b] + live) is loaded: a load of such a row is redirected to the
//     block's last key, which has been written.  A redirected K row only
//     produces scores the mask discards; a redirected V row is replaced by
//     zeros on its way into LDS (0 * NaN is NaN).  Scores of keys at or past
//     min(row limit, block end) become -inf; a wave that has seen no key yet
//     keeps m = -inf under k_attn_decode's guard.
//   * The waves merge through LDS in wave order (the buffer aliases the V
//     slabs, 64 head-dim columns per round).  n_splits == 1 writes bf16
//     O[(b*T + t)][h*D + d]; otherwise fp32 partials (m, l, o[D]) per
//     (b, t, h, s) go to a caller-owned workspace and k_attn_extend_combine
//     folds them in split order.  A row that is not live stores zeros.
//
// No atomics.  The bits of O depend on (inputs, lens, n_new, T, max_len,
// n_splits) only.
#include <hip/hip_runtime.h>
#include <stdint.h>

// packed fp32 VALU forms are kept out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

typedef __bf16 ex_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ex_bf16x2 __attribute__((ext_vector_type(2)));
typedef float ex_f32x16 __attribute__((ext_vector_type(16)));
typedef short ex_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned ex_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ex_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) ex_s16x4 ex_lds_s16x4;

constexpr int EX_NT = 256;    // threads per block
constexpr int EX_NW = 4;      // waves: interleaved key slabs
constexpr int EX_ROWS = 32;   // query rows per block (one MFMA tile)
constexpr int EX_SLAB = 32;   // keys per wave step
constexpr int EX_CHUNK_Q = 64;  // a split's key count is a multiple of this
constexpr int EX_MCOLS = 64;  // head-dim columns per merge round
constexpr float EX_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ---------------------------------------------------------------- rope_kv_extend
// qkv row b*T + t = [H q heads | Hkv k heads | Hkv v heads] x D of new token t
// of batch row b, p = lens[b] + t its position.  k_rope's arithmetic
// (llm_kernels.hip), expression for expression, as k_rope_kv_append: a key
// appended at p is bitwise the key rope_ produces for the same row at p.
// A token that is not live writes nothing and its q columns are left alone.
__global__ __launch_bounds__(EX_NT) void k_rope_kv_extend(uint16_t* qkv, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, uint16_t* __restrict__ kc,
                                                          uint16_t* __restrict__ vc, const int* __restrict__ lens,
                                                          const int* __restrict__ n_new, int B, int T, int H, int Hkv,
                                                          int D, int max_len, int table_len, float sign) {
  const int H2 = D >> 1, Q = H2 >> 2;
  const int nh = H + 2 * Hkv;
  const long long total = (long long)B * T * nh * Q;
  for (long long i = (long long)blockIdx.x * EX_NT + threadIdx.x; i < total; i += (long long)gridDim.x * EX_NT) {
    const int q = (int)(i % Q);
    const long long r = i / Q;
    const int hd = (int)(r % nh);
    const long long bt = r / nh;
    const int b = (int)(bt / T), t = (int)(bt % T);
    const long long pl = (long long)lens[b] + t;
    if (t >= n_new[b] || pl < 0 || pl >= max_len || pl >= table_len) continue;
    const int p = (int)pl;
    const long long off = bt * nh * D + (long long)hd * D + q * 4;
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

// ---------------------------------------------------------------- attn_extend
__device__ __forceinline__ ex_f32x16 mfma(ex_u32x4 a, ex_u32x4 b, ex_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ex_bf16x8, a), __builtin_bit_cast(ex_bf16x8, b), c, 0,
                                                 0, 0);
}

__device__ __forceinline__ unsigned pack2(float a, float b) {
  ex_bf16x2 t = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, t);
}

// Accumulator regs [8s .. 8s+7] of the 32x32 S^T tile (keys along the rows)
// -> the B operand of k-slot s (16 keys) of O^T = V^T P^T: lanes 0-31 need
// keys 16s+0..7, lanes 32-63 keys 16s+8..15; each half holds 4 of them, the
// partner half the rest.
__device__ __forceinline__ ex_u32x4 acc_to_operand(const float* r) {
  unsigned x0 = pack2(r[0], r[1]), x1 = pack2(r[2], r[3]);
  unsigned y0 = pack2(r[4], r[5]), y1 = pack2(r[6], r[7]);
  auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
  auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
  return ex_u32x4{s0[0], s1[0], s0[1], s1[1]};
}

// XOR-swizzled [32 keys][D bf16] image: byte offset of 16-byte chunk ch of key
// row r (attention.hip's image at D = 128; the same pattern cut to the 8
// chunks of a row at D = 64).
template <int D>
__device__ __forceinline__ int swz(int r, int ch) {
  return 2 * D * r + 16 * (ch ^ ((((r & 3) << 2) | ((r >> 2) & 3)) & (D / 8 - 1)));
}

// A operand with k running along the ROWS (keys) of the row-major V slab: two
// transposed reads.  Operand row (d) = col0 + (lane & 31), k = krow0 +
// 8*(lane >> 5) + j.
template <int D>
__device__ __forceinline__ ex_u32x4 tr_operand(const char* tile, int krow0, int col0) {
  const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const int row = krow0 + 8 * (g >> 1) + (li >> 2);
  const int ch = ((col0 + 16 * (g & 1)) >> 3) + ((li & 3) >> 1);
  const char* p0 = tile + swz<D>(row, ch) + 8 * (li & 1);
  const char* p1 = tile + swz<D>(row + 4, ch) + 8 * (li & 1);
  ex_s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ex_lds_s16x4*)p0);
  ex_s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ex_lds_s16x4*)p1);
  ex_u32x2 ua = __builtin_bit_cast(ex_u32x2, a), ub = __builtin_bit_cast(ex_u32x2, b);
  return ex_u32x4{ua[0], ua[1], ub[0], ub[1]};
}

__device__ __forceinline__ ex_u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const ex_u32x4*>(p); }

template <int D>
struct ExLds {
  static constexpr int V_BYTES = EX_NW * EX_SLAB * D * 2;                      // the four private V slabs
  static constexpr int M_BYTES = EX_NW * EX_ROWS * (EX_MCOLS + 1) * 4;         // one merge round, all waves
  static constexpr int BUF = V_BYTES > M_BYTES ? V_BYTES : M_BYTES;
};

// part_ml [B*T][H][n_splits][2] = (m, l), part_o [B*T][H][n_splits][D] fp32.
template <int D, int G>
__global__ __launch_bounds__(EX_NT, 2) void k_attn_extend(const uint16_t* __restrict__ q, long long q_stride,
                                                       const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                       const int* __restrict__ lens, const int* __restrict__ n_new,
                                                       float* __restrict__ part_ml, float* __restrict__ part_o,
                                                       uint16_t* __restrict__ o_direct, long long o_stride, int T, int H,
                                                       int Hkv, int max_len, int chunk, int row_tiles, float sl) {
  constexpr int KS = D / 16;   // k-steps of S^T = 16-byte K loads per lane per slab
  constexpr int DB = D / 32;   // 32-row blocks of O^T
  constexpr int VP = D / 16;   // 16-byte V pieces per lane per slab
  constexpr int CPR = D / 8;   // 16-byte chunks per key row
  constexpr int TPT = EX_ROWS / G;  // tokens per row tile
  __shared__ __attribute__((aligned(16))) char smem[ExLds<D>::BUF];
  __shared__ float sm_m[EX_NW][EX_ROWS], sm_l[EX_NW][EX_ROWS];

  const int s = blockIdx.x, g = blockIdx.y;
  const int b = blockIdx.z / row_tiles, rt = blockIdx.z % row_tiles;
  const int nsplit = gridDim.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, half = lane >> 5, ql = lane & 31;
  const int rows = T * G;

  const long long L = lens[b];
  int nn = n_new[b];
  nn = nn < 0 ? 0 : (nn > T ? T : nn);
  // end of the keys any row of this tile may see: lens[b] + (live tokens up to the tile's last token)
  const int t_last = (rt * TPT + TPT < T) ? rt * TPT + TPT : T;  // one past
  long long endl = L + (nn < t_last ? nn : t_last);
  endl = endl < 0 ? 0 : (endl > max_len ? max_len : endl);
  const int lo = s * chunk;
  const int hi = (lo + chunk < (int)endl) ? lo + chunk : (int)endl;

  if (hi <= lo) {  // uniform over the block: no barrier below is skipped by a part of it
    for (int i = tid; i < EX_ROWS * D; i += EX_NT) {
      const int r = rt * EX_ROWS + i / D, d = i % D;
      if (r >= rows) break;
      const int t = r / G, h = g * G + r % G;
      const long long row = (long long)b * T + t;
      if (o_direct) {
        o_direct[row * o_stride + (long long)h * D + d] = 0;
      } else {
        const long long pr = (row * H + h) * nsplit + s;
        part_o[pr * D + d] = 0.f;
        if (d == 0) {
          part_ml[pr * 2] = -INFINITY;
          part_ml[pr * 2 + 1] = 0.f;
        }
      }
    }
    return;
  }

  // this lane's query row and the first key it may not see (inside this block)
  const int r_q = rt * EX_ROWS + ql;
  const int t_q = r_q / G;
  const long long p_q = L + t_q;
  const bool live = r_q < rows && t_q < nn && p_q >= 0 && p_q < max_len;
  const int lim = live ? (p_q + 1 < hi ? (int)(p_q + 1) : hi) : 0;

  // Q fragments (B operand): row r_q, d = 16*ks + 8*half .. +7; zeros for a row that is not live
  ex_u32x4 qf[KS];
  {
    const uint16_t* qr = q + ((long long)b * T + (live ? t_q : 0)) * q_stride + (long long)(g * G + r_q % G) * D + 8 * half;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const ex_u32x4 v = ld16(qr + 16 * ks);
      qf[ks] = live ? v : ex_u32x4{0, 0, 0, 0};
    }
  }

  ex_f32x16 acc_o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc_o[db] = (ex_f32x16){};
  float m_run = -INFINITY, l_run = 0.f;

  const long long head_off = ((long long)b * Hkv + g) * max_len * D;
  const uint16_t* kb = kc + head_off + 8 * half;            // + key * D + 16 * ks
  const uint16_t* vb = vc + head_off + (lane % CPR) * 8;    // + key * D
  const int vrow = lane / CPR;                              // V piece p: key row vrow + (64 / CPR) * p
  char* vt = smem + w * (EX_SLAB * D * 2);
  const int last = hi - 1;  // hi > lo >= 0: a key this block owns; clamped loads stay on written rows

  // Loads are unconditional and clamped to the block's last key (a conditionally filled register array
  // would be demoted to scratch).  A clamped K row only feeds scores that the mask discards; a clamped V
  // row is replaced by zeros on its way into LDS.
  ex_u32x4 kn[KS], vn[VP];
  auto issue_k = [&](int k0) {
    const int kk = k0 + ql < last ? k0 + ql : last;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kn[ks] = ld16(kb + (long long)kk * D + 16 * ks);
  };
  auto issue_v = [&](int k0) {
#pragma unroll
    for (int p = 0; p < VP; ++p) {
      const int key = k0 + vrow + (64 / CPR) * p;
      vn[p] = ld16(vb + (long long)(key < last ? key : last) * D);
    }
  };
  issue_k(lo + EX_SLAB * w);
  issue_v(lo + EX_SLAB * w);

  for (int k0 = lo + EX_SLAB * w; k0 < hi; k0 += EX_SLAB * EX_NW) {
    // this slab's V to the private LDS slab (rows at or past hi become zeros), then the next slab's V loads
#pragma unroll
    for (int p = 0; p < VP; ++p) {
      const int row = vrow + (64 / CPR) * p;
      *reinterpret_cast<ex_u32x4*>(vt + swz<D>(row, lane % CPR)) = (k0 + row < hi) ? vn[p] : ex_u32x4{0, 0, 0, 0};
    }
    issue_v(k0 + EX_SLAB * EX_NW);  // in flight under this slab's math (the last one re-reads row hi-1)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // S^T: keys along the accumulator rows, the query on the lane; then the next slab's K loads
    ex_f32x16 st = (ex_f32x16){};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) st = mfma(kn[ks], qf[ks], st);
    issue_k(k0 + EX_SLAB * EX_NW);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * half;
      st[i] = key < lim ? st[i] * sl : -INFINITY;
      mx = fmaxf(mx, st[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float ms = (m_new == -INFINITY) ? 0.f : m_new;  // no key yet for this row: everything stays 0
    const float alpha = __builtin_amdgcn_exp2f(m_run - ms);
    float rs = 0.f;
    float pr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      pr[i] = __builtin_amdgcn_exp2f(st[i] - ms);
      rs += pr[i];
    }
    rs += __shfl_xor(rs, 32, 64);
    l_run = l_run * alpha + rs;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc_o[db] *= alpha;
    const ex_u32x4 pf0 = acc_to_operand(pr), pf1 = acc_to_operand(pr + 8);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // O^T += V^T P^T
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      acc_o[db] = mfma(tr_operand<D>(vt, 0, 32 * db), pf0, acc_o[db]);
      acc_o[db] = mfma(tr_operand<D>(vt, 16, 32 * db), pf1, acc_o[db]);
    }
    __builtin_amdgcn_wave_barrier();  // the slab is rewritten only after every lane has read it
  }

  // ---- the four waves, in wave order
  sm_m[w][ql] = m_run;  // both halves hold the same value
  __syncthreads();      // also: every wave is done with its V slab, the merge buffer aliases them
  float M = -INFINITY;
#pragma unroll
  for (int ww = 0; ww < EX_NW; ++ww) M = fmaxf(M, sm_m[ww][ql]);
  {
    const float c = __builtin_amdgcn_exp2f(m_run - ((M == -INFINITY) ? 0.f : M));
    sm_l[w][ql] = l_run * c;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc_o[db] *= c;
  }
  float(*mb)[EX_ROWS][EX_MCOLS + 1] = reinterpret_cast<float(*)[EX_ROWS][EX_MCOLS + 1]>(smem);
#pragma unroll
  for (int rd = 0; rd < D / EX_MCOLS; ++rd) {
    if (rd) __syncthreads();  // the previous round has been folded
#pragma unroll
    for (int dh = 0; dh < EX_MCOLS / 32; ++dh)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        mb[w][ql][32 * dh + (i & 3) + 8 * (i >> 2) + 4 * half] = acc_o[rd * (EX_MCOLS / 32) + dh][i];
    __syncthreads();
    for (int i = tid; i < EX_ROWS * EX_MCOLS; i += EX_NT) {
      const int row = i / EX_MCOLS, dd = i % EX_MCOLS;
      const int r = rt * EX_ROWS + row;
      if (r >= rows) break;  // rows past T*G are never stored
      float Lr = 0.f, O = 0.f, Mr = -INFINITY;
#pragma unroll
      for (int ww = 0; ww < EX_NW; ++ww) {
        Mr = fmaxf(Mr, sm_m[ww][row]);
        Lr += sm_l[ww][row];
        O += mb[ww][row][dd];
      }
      const int t = r / G, h = g * G + r % G, d = rd * EX_MCOLS + dd;
      const long long orow = (long long)b * T + t;
      if (o_direct) {
        o_direct[orow * o_stride + (long long)h * D + d] = f2bf(Lr > 0.f ? O / Lr : 0.f);
      } else {
        const long long pr = (orow * H + h) * nsplit + s;
        part_o[pr * D + d] = O;
        if (d == 0) {
          part_ml[pr * 2] = Mr;
          part_ml[pr * 2 + 1] = Lr;
        }
      }
    }
  }
}

// One block per (b*T + t, h), 128 threads, thread d folds the n_splits
// partials in split order.  A row with no key at all (not live) gives zeros.
__global__ __launch_bounds__(128) void k_attn_extend_combine(const float* __restrict__ part_ml,
                                                             const float* __restrict__ part_o,
                                                             uint16_t* __restrict__ o, long long o_stride, int H, int D,
                                                             int nsplit) {
  const long long rh = blockIdx.x;  // (b*T + t) * H + h
  const int d = threadIdx.x;
  if (d >= D) return;
  const long long r0 = rh * nsplit;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, part_ml[(r0 + s) * 2]);
  const float ms = (M == -INFINITY) ? 0.f : M;
  float L = 0.f, O = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float c = exp2f(part_ml[(r0 + s) * 2] - ms);
    L += part_ml[(r0 + s) * 2 + 1] * c;
    O += part_o[(r0 + s) * D + d] * c;
  }
  o[(rh / H) * o_stride + (rh % H) * D + d] = f2bf(L > 0.f ? O / L : 0.f);
}

template <int D>
int launch_extend(int G, dim3 grid, hipStream_t s, const uint16_t* q, long long q_stride, const uint16_t* kc,
                  const uint16_t* vc, const int* lens, const int* n_new, float* part_ml, float* part_o,
                  uint16_t* o_direct, long long o_stride, int T, int H, int Hkv, int max_len, int chunk, int row_tiles,
                  float sl) {
#define PTO_EXTEND_CASE(GG)                                                                                          \
  case GG:                                                                                                           \
    hipLaunchKernelGGL((k_attn_extend<D, GG>), grid, dim3(EX_NT), 0, s, q, q_stride, kc, vc, lens, n_new, part_ml,   \
                       part_o, o_direct, o_stride, T, H, Hkv, max_len, chunk, row_tiles, sl);                        \
    break;
  switch (G) {
    PTO_EXTEND_CASE(1)
    PTO_EXTEND_CASE(2)
    PTO_EXTEND_CASE(4)
    PTO_EXTEND_CASE(8)
    default:
      return -1;
  }
#undef PTO_EXTEND_CASE
  return 0;
}

}  // namespace

#pragma clang attribute pop

#define PTO_API extern "C" __attribute__((visibility("default")))

// qkv [B*T][(H + 2*Hkv)*D] bf16 contiguous, cs/sn fp32 [table_len][D/2],
// k_cache/v_cache bf16 [B][Hkv][max_len][D], lens / n_new int32 [B].
PTO_API int pto_rope_kv_extend(void* qkv, const float* cs, const float* sn, void* k_cache, void* v_cache,
                               const int* lens, const int* n_new, int B, int T, int H, int Hkv, int D, int max_len,
                               int table_len, hipStream_t s) {
  if (D % 8 || B < 0 || T < 0 || H < 1 || Hkv < 1 || max_len < 1 || table_len < 1) return -1;
  if (B == 0 || T == 0) return 0;
  long long blocks = ((long long)B * T * (H + 2 * Hkv) * (D / 8) + EX_NT - 1) / EX_NT;
  if (blocks > 65535) blocks = 65535;
  hipLaunchKernelGGL(k_rope_kv_extend, dim3((unsigned)blocks), dim3(EX_NT), 0, s, (uint16_t*)qkv, cs, sn,
                     (uint16_t*)k_cache, (uint16_t*)v_cache, lens, n_new, B, T, H, Hkv, D, max_len, table_len, 1.f);
  return (int)hipGetLastError();
}

PTO_API int pto_attn_extend_supported(int H, int Hkv, int D) {
  if (H < 1 || Hkv < 1 || H % Hkv) return 0;
  const int G = H / Hkv;
  return (D == 64 || D == 128) && (G == 1 || G == 2 || G == 4 || G == 8);
}

// Keys per split: fixed by max_len and n_splits alone, a multiple of 64.
PTO_API int pto_attn_extend_chunk(int max_len, int n_splits) {
  if (max_len < 1 || n_splits < 1) return -1;
  const int c = (max_len + n_splits - 1) / n_splits;
  return (c + EX_CHUNK_Q - 1) / EX_CHUNK_Q * EX_CHUNK_Q;
}

// q: the new rows' (rotated) query heads, bf16, head h of row b*T + t at
// q + (b*T + t)*q_stride + h*D (elements); o bf16 [B*T][H*D].  part_ml /
// part_o: fp32 workspaces of B*T*H*n_splits*2 and B*T*H*n_splits*D floats
// (unused when n_splits == 1).
PTO_API int pto_attn_extend(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                            const int* lens, const int* n_new, void* o, float* part_ml, float* part_o, int B, int T,
                            int H, int Hkv, int D, int max_len, int n_splits, float scale, hipStream_t s) {
  if (!pto_attn_extend_supported(H, Hkv, D) || max_len < 1 || n_splits < 1 || n_splits > 65535 || Hkv > 65535 ||
      B < 0 || T < 0 || (q_stride % 8) ||
      ((((uintptr_t)q) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache) | ((uintptr_t)o)) & 15))
    return -1;
  if (B == 0 || T == 0) return 0;
  const int G = H / Hkv;
  const long long row_tiles = ((long long)T * G + EX_ROWS - 1) / EX_ROWS;
  if (B * row_tiles > 65535 || (long long)B * T * H > 2147483647LL) return -1;
  if (n_splits > 1 && (!part_ml || !part_o)) return -1;
  const int chunk = pto_attn_extend_chunk(max_len, n_splits);
  const float sl = scale * EX_LOG2E;
  uint16_t* od = n_splits == 1 ? (uint16_t*)o : nullptr;
  const dim3 grid(n_splits, Hkv, (unsigned)(B * row_tiles));
  const long long o_stride = (long long)H * D;
  int rc;
  if (D == 128)
    rc = launch_extend<128>(G, grid, s, (const uint16_t*)q, q_stride, (const uint16_t*)k_cache,
                            (const uint16_t*)v_cache, lens, n_new, part_ml, part_o, od, o_stride, T, H, Hkv, max_len,
                            chunk, (int)row_tiles, sl);
  else
    rc = launch_extend<64>(G, grid, s, (const uint16_t*)q, q_stride, (const uint16_t*)k_cache,
                           (const uint16_t*)v_cache, lens, n_new, part_ml, part_o, od, o_stride, T, H, Hkv, max_len,
                           chunk, (int)row_tiles, sl);
  if (rc) return rc;
  if (n_splits > 1)
    hipLaunchKernelGGL(k_attn_extend_combine, dim3((unsigned)((long long)B * T * H)), dim3(128), 0, s, part_ml, part_o,
                       (uint16_t*)o, o_stride, H, D, n_splits);
  return (int)hipGetLastError();
}
