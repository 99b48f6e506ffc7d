// Weight-only MX (OCP microscaling) skinny GEMM for the decode-time linear
// layers (ops/gemm.py skinny_mx_nt, models/llama.py Llama.quantize_weights):
//
//     y[M,N] = x[M,K] . dequant(Wq)[N,K]^T      1 <= M <= 16, x bf16, fp32 sums,
//
// Wq in MXFP4 (e2m1, two elements per byte, element 2i in the low nibble of
// byte i) or MXFP8 (e4m3fn), one E8M0 scale byte e (2^(e-127), 1 <= e <= 254)
// per block of 32 consecutive K elements of a row: data uint8 [N][K/2] or
// [N][K], scales uint8 [N][K/32], both contiguous.  Dequantisation to bf16 is
// exact (at most 3 mantissa bits times a power of two), so the product is the
// bf16 kernel's (gemm_skinny.hip) on 4.25 or 8.25 bits per weight.
//
//   * v_mfma_f32_16x16x32_bf16, 16 weight rows the A operand and x (rows
//     m >= M zero) the B operand, with K permuted so that the weight loads are
//     wide: inside a group of 512 K elements (16 MX blocks) lane (r = l%16,
//     kq = l/16) owns the blocks 4*kq .. 4*kq+3 of row n0 + r -- 64 contiguous
//     bytes of fp4 (four 16-byte loads), 128 of fp8, and ONE aligned 4-byte
//     load of scales.  A wave's loads of a group cover 256 (512) contiguous
//     bytes of each of 16 rows: whole cache lines.  Block u of a lane gives
//     four 8-element operand chunks; MFMA (u, j) contracts chunk j of block u
//     against the x chunk at the same K positions (the contraction does not
//     care which 32 K positions an MFMA sees as long as A and B agree).
//   * Unpack: v_cvt_scalef32_pk_bf16_fp4 / _fp8 with the block's scale as the
//     fp32 bit pattern e << 23: two elements per instruction, already bf16.
//   * x goes through LDS.  A workgroup (4 waves) walks ONE K range; its waves
//     split N, two row tiles each (plain: 32 consecutive rows; SwiGLU: a gate
//     tile and its up tile F + n).  The x slice of a group (16 x 512 bf16) is
//     staged by all 256 threads, double buffered, one barrier per group, laid
//     out chunk-major -- slot ((u*4 + j)*4 + kq)*16 + m of 16 bytes -- so the
//     64 lanes' reads of one MFMA's operand are 1024 contiguous bytes.  Rows
//     m >= M are zero-filled once and never loaded; chunks past K are zeros.
//     The next group's weights and x are loaded into registers before the
//     current group's MFMAs.  No cross-wave reduction exists.
//   * K across workgroups: blockIdx.y = split s takes the groups
//     [s*per, (s+1)*per), per = ceil(groups / n_splits); with n_splits > 1 the
//     fp32 tiles go to ws[s][m][n] (the caller's workspace) and a second small
//     launch adds them in split order.  No atomics, counters, allocation or
//     sync: the pair captures into a graph.
//
// Bits: output (m, n) is a function of x[m], row n of the quantised weight, K
// and n_splits alone: the group-to-split map does not look at M or N, a wave
// sums its groups in order, an MFMA column does not depend on the others.
// SwiGLU is k_swiglu_fwd's arithmetic on the bf16-rounded gate and up, so
// bitwise ops.llm.swiglu of the plain bf16 result.
//
// k_quant_mx is the quantiser (OCP MX v1.0): per block e = clamp(floor(log2(
// amax)) - emax + 127, 1, 254) (127 for amax == 0), elements w / 2^(e-127)
// rounded to nearest even on the element grid, saturating.  Plain C++: the
// same comparisons as ops/gemm.py's torch reference, byte for byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

// packed fp32 VALU forms are kept out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

typedef __bf16 mx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mx_bf16x2 __attribute__((ext_vector_type(2)));
typedef float mx_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned mx_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned mx_u32x2 __attribute__((ext_vector_type(2)));

constexpr int MX_T = 256;            // threads per workgroup
constexpr int MX_GROUP = 512;        // K elements of a group: 16 MX blocks, 4 per lane quarter
constexpr int MX_SLOTS = 16 * 64;    // 16-byte slots of one staged x slice (16 rows x 512 bf16)
constexpr int MX_MAX_SPLITS = 64;

enum { EPI_PLAIN = 0, EPI_SWIGLU = 1 };
enum { FMT_FP4 = 0, FMT_FP8 = 1 };

__device__ __forceinline__ float bf2f(uint16_t x) { return __uint_as_float(((uint32_t)x) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {  // round to nearest even
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }
// k_swiglu_fwd's expression on bf16-rounded gate and up
__device__ __forceinline__ uint16_t swiglu1(float g, float u) {
  const float gr = bf2f(f2bf(g)), ur = bf2f(f2bf(u));
  return f2bf(bf2f(f2bf(gr * sigmoidf(gr))) * ur);
}

__device__ __forceinline__ mx_f32x4 mfma(mx_u32x4 a, mx_u32x4 b, mx_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mx_bf16x8, a), __builtin_bit_cast(mx_bf16x8, b), c,
                                                 0, 0, 0);
}

// Four consecutive columns of one output row.
__device__ __forceinline__ void store4(void* out, int out_f32, long long idx, mx_f32x4 v) {
  if (out_f32) {
    *reinterpret_cast<mx_f32x4*>((float*)out + idx) = v;
  } else {
    mx_u32x2 p;
    p.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
    p.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
    *reinterpret_cast<mx_u32x2*>((uint16_t*)out + idx) = p;
  }
}
__device__ __forceinline__ void store4_swiglu(uint16_t* out, long long idx, mx_f32x4 g, mx_f32x4 u) {
  mx_u32x2 p;
  p.x = (uint32_t)swiglu1(g.x, u.x) | ((uint32_t)swiglu1(g.y, u.y) << 16);
  p.y = (uint32_t)swiglu1(g.z, u.z) | ((uint32_t)swiglu1(g.w, u.w) << 16);
  *reinterpret_cast<mx_u32x2*>(out + idx) = p;
}

// ---------------------------------------------------------------- weights of one lane, one group
// 4 blocks of one row: 4 (fp4) or 8 (fp8) 16-byte vectors and the 4 scale bytes.
template <int FMT>
struct WRegs {
  static constexpr int NV = FMT == FMT_FP4 ? 4 : 8;
  mx_u32x4 q[NV];
  uint32_t sc;
};

// dp / sp: the lane's row and quarter, group 0.  !ok (no such tile, or the
// quarter lies past K in the last group): zeros, nothing is read.
template <int FMT>
__device__ __forceinline__ void load_w(WRegs<FMT>& r, const uint8_t* dp, const uint8_t* sp, long long g, bool ok) {
  constexpr int NV = WRegs<FMT>::NV;
  const mx_u32x4* p = reinterpret_cast<const mx_u32x4*>(dp + g * (NV * 64));
#pragma unroll
  for (int i = 0; i < NV; ++i) r.q[i] = ok ? p[i] : mx_u32x4{0u, 0u, 0u, 0u};
  r.sc = ok ? *reinterpret_cast<const uint32_t*>(sp + g * 16) : 0x7f7f7f7fu;
}

__device__ __forceinline__ uint32_t pk(mx_bf16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// Chunk j (8 elements) of block u as the bf16 MFMA operand, scaled by s.
template <int FMT>
__device__ __forceinline__ mx_u32x4 unpack(const WRegs<FMT>& r, int u, int j, float s) {
  mx_u32x4 o;
  if (FMT == FMT_FP4) {  // one dword = 8 nibbles; byte b holds elements 2b (low nibble), 2b+1
    const uint32_t d = r.q[u][j];
    o.x = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0));
    o.y = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1));
    o.z = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2));
    o.w = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3));
  } else {  // two dwords = 8 bytes
    const uint32_t d0 = r.q[2 * u + (j >> 1)][2 * (j & 1)], d1 = r.q[2 * u + (j >> 1)][2 * (j & 1) + 1];
    o.x = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, s, false));
    o.y = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, s, true));
    o.z = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, s, false));
    o.w = pk(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, s, true));
  }
  return o;
}

// The 16 MFMAs of a group for both tiles of a wave; xl = the lane's slot of
// MFMA (0, 0) in the staged slice, MFMA (u, j) is 64 slots further each.
template <int FMT>
__device__ __forceinline__ void group_mfma(const WRegs<FMT>& a, const WRegs<FMT>& b, const mx_u32x4* xl, mx_f32x4& accA,
                                           mx_f32x4& accB) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float sa = __uint_as_float(((a.sc >> (8 * u)) & 255u) << 23);
    const float sb = __uint_as_float(((b.sc >> (8 * u)) & 255u) << 23);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const mx_u32x4 xv = xl[(u * 4 + j) * 64];
      accA = mfma(unpack<FMT>(a, u, j, sa), xv, accA);
      accB = mfma(unpack<FMT>(b, u, j, sb), xv, accB);
    }
  }
}

// ---------------------------------------------------------------- x staging
// Thread (m = tid%16, cb = tid/16) moves the chunks c = cb + 16*i (i = 0..3 is
// the lane quarter kq, cb the MFMA index u*4 + j) of row m: 16 bytes each.
struct XRegs {
  mx_u32x4 v[4];
};
__device__ __forceinline__ void load_x(XRegs& r, const uint16_t* xp, long long g, int cb, int K) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long k = g * MX_GROUP + (i * 16 + cb) * 8;
    r.v[i] = k < K ? *reinterpret_cast<const mx_u32x4*>(xp + k) : mx_u32x4{0u, 0u, 0u, 0u};
  }
}
__device__ __forceinline__ void store_x(mx_u32x4* buf, const XRegs& r, int m, int cb) {
#pragma unroll
  for (int i = 0; i < 4; ++i) buf[(cb * 4 + i) * 16 + m] = r.v[i];
}

// Grid (row spans of 128 rows -- 64 gate rows with SwiGLU --, n_splits), 256 threads.
template <int FMT, int EPI>
__global__ __launch_bounds__(MX_T) void k_gemm_skinny_mx(const uint16_t* __restrict__ x, long long lda,
                                                         const uint8_t* __restrict__ data,
                                                         const uint8_t* __restrict__ scales, void* out, long long ldc,
                                                         int out_f32, float* __restrict__ ws, int M, int N, int K,
                                                         int per) {
  __shared__ mx_u32x4 xs[2][MX_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int F = N >> 1;
  // the two row tiles of this wave; has* are uniform over the wave
  const int nA = EPI == EPI_SWIGLU ? blockIdx.x * 64 + wv * 16 : blockIdx.x * 128 + wv * 32;
  const int nB = EPI == EPI_SWIGLU ? F + nA : nA + 16;
  const bool hasA = EPI == EPI_SWIGLU ? nA < F : nA < N;
  const bool hasB = EPI == EPI_SWIGLU ? hasA : nB < N;
  const int groups = (K + MX_GROUP - 1) / MX_GROUP;
  const int lo = blockIdx.y * per;
  const int hi = lo + per < groups ? lo + per : groups;

  constexpr int ROWB = FMT == FMT_FP4 ? 2 : 1;  // K elements per data byte
  const long long row_bytes = K / ROWB, row_scales = K >> 5;
  const uint8_t* da = data + (long long)((hasA ? nA : 0) + r16) * row_bytes + kq * (128 / ROWB);
  const uint8_t* db = data + (long long)((hasB ? nB : 0) + r16) * row_bytes + kq * (128 / ROWB);
  const uint8_t* sa = scales + (long long)((hasA ? nA : 0) + r16) * row_scales + kq * 4;
  const uint8_t* sb = scales + (long long)((hasB ? nB : 0) + r16) * row_scales + kq * 4;

  const int xm = tid & 15, xc = tid >> 4;
  const bool xrow = xm < M;
  const uint16_t* xp = x + (long long)(xrow ? xm : 0) * lda;

  WRegs<FMT> ca, cb, na, nb;
  XRegs xr;
  if (lo < hi) {
    const bool kok = (long long)lo * MX_GROUP + kq * 128 < K;
    load_w<FMT>(ca, da, sa, lo, hasA && kok);
    load_w<FMT>(cb, db, sb, lo, hasB && kok);
    if (xrow) load_x(xr, xp, lo, xc, K);
  }
  if (!xrow) {  // rows m >= M of both buffers: zero once
    const XRegs z = {{{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}};
    store_x(xs[0], z, xm, xc);
    store_x(xs[1], z, xm, xc);
  } else if (lo < hi) {
    store_x(xs[0], xr, xm, xc);
  }
  __syncthreads();

  mx_f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
  for (int g = lo; g < hi; ++g) {
    const int b = (g - lo) & 1;
    const bool more = g + 1 < hi;  // uniform over the workgroup
    if (more) {
      const bool kok = (long long)(g + 1) * MX_GROUP + kq * 128 < K;
      load_w<FMT>(na, da, sa, g + 1, hasA && kok);
      load_w<FMT>(nb, db, sb, g + 1, hasB && kok);
      if (xrow) load_x(xr, xp, g + 1, xc, K);
    }
    group_mfma<FMT>(ca, cb, xs[b] + lane, accA, accB);
    if (more) {
      // xs[b ^ 1] was last read before the barrier that ended group g - 1
      if (xrow) store_x(xs[b ^ 1], xr, xm, xc);
      ca = na;
      cb = nb;
    }
    __syncthreads();
  }

  if (r16 >= M) return;  // rows m >= M: nothing is written
  const int m = r16, c = kq * 4;
  if (ws) {  // fp32 partial tiles of this split, [n_splits][M][N]
    float* p = ws + ((long long)blockIdx.y * M + m) * N;
    if (hasA) *reinterpret_cast<mx_f32x4*>(p + nA + c) = accA;
    if (hasB) *reinterpret_cast<mx_f32x4*>(p + nB + c) = accB;
  } else if (EPI == EPI_SWIGLU) {
    if (hasA) store4_swiglu((uint16_t*)out, (long long)m * ldc + nA + c, accA, accB);
  } else {
    if (hasA) store4(out, out_f32, (long long)m * ldc + nA + c, accA);
    if (hasB) store4(out, out_f32, (long long)m * ldc + nB + c, accB);
  }
}

// The splits of ws [n_splits][M][N] in split order, then the epilogue; one
// thread per four output columns of a row.
template <int EPI>
__global__ __launch_bounds__(MX_T) void k_gemm_skinny_mx_reduce(const float* __restrict__ ws, void* out, long long ldc,
                                                                int out_f32, int M, int N, int n_splits) {
  const int cols = EPI == EPI_SWIGLU ? N >> 1 : N;
  const int q = cols >> 2;
  const int i = blockIdx.x * MX_T + threadIdx.x;
  if (i >= M * q) return;
  const int m = i / q, c = (i - m * q) * 4;
  const long long plane = (long long)M * N;
  const float* p = ws + (long long)m * N + c;
  mx_f32x4 g = *reinterpret_cast<const mx_f32x4*>(p), u = {0.f, 0.f, 0.f, 0.f};
  if (EPI == EPI_SWIGLU) u = *reinterpret_cast<const mx_f32x4*>(p + cols);
  for (int s = 1; s < n_splits; ++s) {
    g += *reinterpret_cast<const mx_f32x4*>(p + s * plane);
    if (EPI == EPI_SWIGLU) u += *reinterpret_cast<const mx_f32x4*>(p + s * plane + cols);
  }
  if (EPI == EPI_SWIGLU)
    store4_swiglu((uint16_t*)out, (long long)m * ldc + c, g, u);
  else
    store4(out, out_f32, (long long)m * ldc + c, g);
}

// ---------------------------------------------------------------- quantiser
// e2m1 code of |v| on the grid {0, .5, 1, 1.5, 2, 3, 4, 6}: the number of
// midpoints below it, a tie going to the even code; saturates at 6.
__device__ __forceinline__ uint32_t quant_fp4(float v) {
  const float a = fabsf(v);
  const uint32_t code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
  return code | ((__float_as_uint(v) >> 28) & 8u);
}
// e4m3fn bits of v, round to nearest even, saturating at 448.
__device__ __forceinline__ uint32_t quant_fp8(float v) {
  const float a = fminf(fabsf(v), 448.f);
  uint32_t code;
  if (a < 0.015625f) {  // below the smallest normal 2^-6: multiples of 2^-9
    code = (uint32_t)rintf(a * 512.f);
  } else {
    uint32_t u = __float_as_uint(a);
    u += 0x7ffffu + ((u >> 20) & 1u);
    code = (u >> 20) - (120u << 3);
  }
  return code | ((__float_as_uint(v) >> 24) & 0x80u);
}

// One thread per 8 elements, four neighbouring lanes per MX block.
template <int FMT>
__global__ __launch_bounds__(MX_T) void k_quant_mx(const uint16_t* __restrict__ w, long long ldw,
                                                   uint8_t* __restrict__ data, uint8_t* __restrict__ scales, int N,
                                                   int K) {
  const long long per_row = K >> 3;
  const long long i = (long long)blockIdx.x * MX_T + threadIdx.x;
  if (i >= N * per_row) return;  // whole blocks of four lanes leave together
  const long long n = i / per_row;
  const int c8 = (int)(i - n * per_row);
  const mx_u32x4 raw = *reinterpret_cast<const mx_u32x4*>(w + n * ldw + c8 * 8);
  float v[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(raw[j] << 16);
    v[2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u);
  }
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  // floor(log2(amax)) + 127 is the exponent field (a subnormal amax clamps to e = 1 either way)
  int e = (int)((__float_as_uint(amax) >> 23) & 255u) - (FMT == FMT_FP4 ? 2 : 8);
  e = e < 1 ? 1 : (e > 254 ? 254 : e);
  if (amax == 0.f) e = 127;
  const float inv = __uint_as_float((uint32_t)(254 - e) << 23);  // 2^(127 - e), exact
  if (FMT == FMT_FP4) {
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) p |= quant_fp4(v[j] * inv) << (4 * j);
    *reinterpret_cast<uint32_t*>(data + n * (K >> 1) + c8 * 4) = p;
  } else {
    mx_u32x2 p = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p.x |= quant_fp8(v[j] * inv) << (8 * j);
      p.y |= quant_fp8(v[4 + j] * inv) << (8 * j);
    }
    *reinterpret_cast<mx_u32x2*>(data + n * (long long)K + c8 * 8) = p;
  }
  if ((c8 & 3) == 0) scales[n * (K >> 5) + (c8 >> 2)] = (uint8_t)e;
}

}  // namespace

#pragma clang attribute pop

#define PTO_API extern "C" __attribute__((visibility("default")))

// The shape rules alone (contiguous operands): fmt 0 (mxfp4) or 1 (mxfp8),
// 1 <= M <= 16, N % 16 == 0 (N % 32 == 0 for swiglu), K % 128 == 0.
PTO_API int pto_gemm_skinny_mx_supported(int epilogue, int fmt, long long M, long long N, long long K) {
  if (epilogue != EPI_PLAIN && epilogue != EPI_SWIGLU) return 0;
  if (fmt != FMT_FP4 && fmt != FMT_FP8) return 0;
  if (M < 1 || M > 16 || N < 16 || K < 128 || K % 128 || K > (1LL << 30)) return 0;
  if (N % (epilogue == EPI_SWIGLU ? 32 : 16) || N > (1LL << 24)) return 0;
  return 1;
}

// Default K split across workgroups, a function of (N, K, fmt) alone: enough
// workgroups for two per compute unit of a 256-CU device while a split keeps
// at least two groups, so that its register prefetch has something to hide.
PTO_API int pto_gemm_skinny_mx_splits(long long N, long long K, int fmt) {
  (void)fmt;
  if (N < 16 || K < 128) return 1;
  const long long spans = (N + 127) / 128, groups = (K + MX_GROUP - 1) / MX_GROUP;
  long long ns = (512 + spans - 1) / spans;
  if (ns > groups / 2) ns = groups / 2;
  if (ns > 16) ns = 16;
  return ns < 1 ? 1 : (int)ns;
}

// Bytes of fp32 partials a call needs (0 for n_splits == 1).
PTO_API long long pto_gemm_skinny_mx_workspace(long long M, long long N, int n_splits) {
  if (M < 1 || N < 1 || n_splits < 1) return -1;
  return n_splits == 1 ? 0 : (long long)n_splits * M * N * 4;
}

// x bf16 [M][K] (row stride lda elements), data / scales the contiguous MX
// weight [N][K] in format fmt, out [M][N] bf16 or fp32 (out_f32; row stride
// ldc), or bf16 [M][N/2] = silu(gate) * up for epilogue 1 (rows [gate; up]).
// ws: ws_bytes of device memory for the fp32 partials when n_splits > 1.
// Returns -1, having launched nothing, on anything outside the rules.
PTO_API int pto_gemm_skinny_mx(const void* x, long long lda, const void* data, const void* scales, void* out,
                               long long ldc, int out_f32, int epilogue, int fmt, int M, int N, int K, int n_splits,
                               void* ws, long long ws_bytes, hipStream_t s) {
  if (!pto_gemm_skinny_mx_supported(epilogue, fmt, M, N, K)) return -1;
  const int cols = epilogue == EPI_SWIGLU ? N / 2 : N;
  if (epilogue == EPI_SWIGLU && out_f32) return -1;
  if (lda < K || ldc < cols || lda % 8 || ldc % 8) return -1;
  if (!x || !data || !scales || !out) return -1;
  if ((((uintptr_t)x) | ((uintptr_t)data) | ((uintptr_t)scales) | ((uintptr_t)out)) & 15) return -1;
  if (n_splits < 1 || n_splits > MX_MAX_SPLITS) return -1;
  float* part = nullptr;
  if (n_splits > 1) {
    if (!ws || (((uintptr_t)ws) & 15) || ws_bytes < pto_gemm_skinny_mx_workspace(M, N, n_splits)) return -1;
    part = (float*)ws;
  }
  const int groups = (K + MX_GROUP - 1) / MX_GROUP;
  const int per = (groups + n_splits - 1) / n_splits;
  const dim3 grid(epilogue == EPI_SWIGLU ? (N / 2 + 63) / 64 : (N + 127) / 128, n_splits);
  const dim3 rgrid((unsigned)((M * (cols / 4) + MX_T - 1) / MX_T));
  const uint16_t* xp = (const uint16_t*)x;
  const uint8_t *dp = (const uint8_t*)data, *sp = (const uint8_t*)scales;
#define MX_LAUNCH(FMT, EPI, F32)                                                                                  \
  hipLaunchKernelGGL((k_gemm_skinny_mx<FMT, EPI>), grid, dim3(MX_T), 0, s, xp, lda, dp, sp, out, ldc, F32, part, M, N, \
                     K, per)
  if (epilogue == EPI_SWIGLU) {
    if (fmt == FMT_FP4)
      MX_LAUNCH(FMT_FP4, EPI_SWIGLU, 0);
    else
      MX_LAUNCH(FMT_FP8, EPI_SWIGLU, 0);
    if (part)
      hipLaunchKernelGGL(k_gemm_skinny_mx_reduce<EPI_SWIGLU>, rgrid, dim3(MX_T), 0, s, part, out, ldc, 0, M, N,
                         n_splits);
  } else {
    if (fmt == FMT_FP4)
      MX_LAUNCH(FMT_FP4, EPI_PLAIN, out_f32);
    else
      MX_LAUNCH(FMT_FP8, EPI_PLAIN, out_f32);
    if (part)
      hipLaunchKernelGGL(k_gemm_skinny_mx_reduce<EPI_PLAIN>, rgrid, dim3(MX_T), 0, s, part, out, ldc, out_f32, M, N,
                         n_splits);
  }
#undef MX_LAUNCH
  return (int)hipGetLastError();
}

// w bf16 [N][K] (row stride ldw elements, a multiple of 8; 16-byte aligned)
// -> data uint8 [N][K/2] (fmt 0) or [N][K] (fmt 1) and scales uint8 [N][K/32],
// contiguous; K % 32 == 0.  Returns -1, having launched nothing, otherwise.
PTO_API int pto_quant_mx(const void* w, long long ldw, void* data, void* scales, int fmt, long long N, long long K,
                         hipStream_t s) {
  if (fmt != FMT_FP4 && fmt != FMT_FP8) return -1;
  if (N < 1 || K < 32 || K % 32 || N > (1LL << 24) || K > (1LL << 30) || ldw < K || ldw % 8) return -1;
  if (!w || !data || !scales || ((((uintptr_t)w) | ((uintptr_t)data)) & 15)) return -1;
  const long long threads = N * (K / 8);
  if (threads > (1LL << 38)) return -1;
  const dim3 grid((unsigned)((threads + MX_T - 1) / MX_T));
  if (fmt == FMT_FP4)
    hipLaunchKernelGGL(k_quant_mx<FMT_FP4>, grid, dim3(MX_T), 0, s, (const uint16_t*)w, ldw, (uint8_t*)data,
                       (uint8_t*)scales, (int)N, (int)K);
  else
    hipLaunchKernelGGL(k_quant_mx<FMT_FP8>, grid, dim3(MX_T), 0, s, (const uint16_t*)w, ldw, (uint8_t*)data,
                       (uint8_t*)scales, (int)N, (int)K);
  return (int)hipGetLastError();
}
