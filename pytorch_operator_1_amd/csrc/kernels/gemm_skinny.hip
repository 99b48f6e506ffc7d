// Skinny bf16 GEMM for the decode-time linear layers (ops/gemm.py skinny_nt,
// models/llama.py LlamaBlock.decode):
//
//     y[M,N] = x[M,K] . W[N,K]^T        1 <= M <= 16, fp32 sums,
//
// with W read exactly as nn.Linear stores it.  At M <= 16 the product is pure
// weight streaming (2*M FLOP per weight byte), so the kernel is built around
// the W loads and nothing else:
//
//   * v_mfma_f32_16x16x32_bf16.  The 16 W rows of a tile are the A operand,
//     x (rows m >= M fed as zeros) the B operand: lane l of a wave holds
//     W[n0 + l%16][k0 + 8*(l/16) .. +8] and x[l%16][k0 + 8*(l/16) .. +8].
//     Each is ONE 16-byte global load that is already the MFMA operand, so W
//     never passes through LDS (nor does x: it is at most 16 rows, shared by
//     every wave of the grid, and is read through L2).  W loads are plain
//     loads: a load instruction covers 64 bytes of each of 16 rows, half a
//     cache line, and the next step's load wants the other half, so a
//     non-temporal hint costs about 10% (profiles/decode_linear.md).  The
//     result tile is D[n][m]: lane l holds n = n0 + 4*(l/16) + r (r = 0..3), m = l%16 --
//     four consecutive output columns of one row, one 8- or 16-byte store.
//   * A workgroup (4 waves) owns TWO row tiles that share the x operand:
//     rows n..n+15 and n+16..n+31 for the plain epilogue, gate rows n..n+15
//     and up rows F+n..F+n+15 for the SwiGLU one.  One x load feeds two MFMAs.
//   * K is cut three ways.  blockIdx.y = split s of n_splits takes the steps
//     (of 32 elements) [s*per, (s+1)*per), per = ceil(K/32 / n_splits); inside
//     a split the waves take groups of SK_U consecutive steps round robin
//     (wave w: groups w, w+4, ...), and every wave issues the 3*SK_U loads of
//     a group before the first MFMA of it.  Ranges that the waves or splits
//     do not divide evenly end in a guarded group; an empty range sums to 0.
//   * The four partial tiles of a workgroup meet in LDS and wave 0 adds them
//     in wave order.  With n_splits == 1 it applies the epilogue; otherwise
//     it stores the fp32 tile to ws[s][m][n] (workspace handed in by the
//     caller) and a second small launch adds the splits in split order.
//     No atomics, no counters, no allocation, no sync: the pair of launches
//     captures into a graph.
//
// Bits: output (m, n) is a function of x[m], W[n], K and n_splits alone --
// the step-to-wave and step-to-split maps do not look at M or N, an MFMA
// column does not depend on the other columns, and all sums have a fixed
// order.  The SwiGLU epilogue is k_swiglu_fwd's arithmetic (llm_kernels.hip)
// on the bf16-rounded gate and up, so it is bitwise ops.llm.swiglu of the
// plain bf16 result.  Only the M x N (M x F) result is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

// packed fp32 VALU forms are kept out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

typedef __bf16 sk_bf16x8 __attribute__((ext_vector_type(8)));
typedef float sk_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned sk_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned sk_u32x2 __attribute__((ext_vector_type(2)));

constexpr int SK_T = 256;        // threads per workgroup
constexpr int SK_W = SK_T / 64;  // waves: the K cut inside a workgroup
constexpr int SK_U = 4;          // K steps per group = loads of one W tile in flight per wave
constexpr int SK_MAX_SPLITS = 64;

enum { EPI_PLAIN = 0, EPI_SWIGLU = 1 };

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

__device__ __forceinline__ sk_u32x4 ldw(const uint16_t* p) { return *reinterpret_cast<const sk_u32x4*>(p); }
__device__ __forceinline__ sk_f32x4 mfma(sk_u32x4 a, sk_u32x4 b, sk_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sk_bf16x8, a), __builtin_bit_cast(sk_bf16x8, b), c,
                                                 0, 0, 0);
}

// Four consecutive columns of one output row.
__device__ __forceinline__ void store4(void* out, int out_f32, long long idx, sk_f32x4 v) {
  if (out_f32) {
    *reinterpret_cast<sk_f32x4*>((float*)out + idx) = v;
  } else {
    sk_u32x2 p;
    p.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
    p.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
    *reinterpret_cast<sk_u32x2*>((uint16_t*)out + idx) = p;
  }
}
__device__ __forceinline__ void store4_swiglu(uint16_t* out, long long idx, sk_f32x4 g, sk_f32x4 u) {
  sk_u32x2 p;
  p.x = (uint32_t)swiglu1(g.x, u.x) | ((uint32_t)swiglu1(g.y, u.y) << 16);
  p.y = (uint32_t)swiglu1(g.z, u.z) | ((uint32_t)swiglu1(g.w, u.w) << 16);
  *reinterpret_cast<sk_u32x2*>(out + idx) = p;
}

// Grid (tile pairs, n_splits), 256 threads.  A plain pair whose second tile
// starts at N (N/16 odd) has no second tile.
template <int EPI>
__global__ __launch_bounds__(SK_T) void k_gemm_skinny(const uint16_t* __restrict__ x, long long lda,
                                                      const uint16_t* __restrict__ w, long long ldb, void* out,
                                                      long long ldc, int out_f32, float* __restrict__ ws, int M, int N,
                                                      int K, int per) {
  __shared__ sk_f32x4 red[SK_W][2][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int F = N >> 1;
  // the two row tiles of this workgroup
  const int nA = EPI == EPI_SWIGLU ? blockIdx.x * 16 : blockIdx.x * 32;
  const int nB = EPI == EPI_SWIGLU ? F + nA : nA + 16;
  const bool hasB = nB < N;  // plain: N/16 may be odd; uniform over the workgroup
  const int steps = K >> 5;
  const int lo = blockIdx.y * per;
  const int hi = lo + per < steps ? lo + per : steps;

  const uint16_t* wa = w + (long long)(nA + r16) * ldb + kq * 8;
  const uint16_t* wb = w + (long long)((hasB ? nB : nA) + r16) * ldb + kq * 8;
  const bool xrow = r16 < M;
  const uint16_t* xp = x + (long long)(xrow ? r16 : 0) * lda + kq * 8;
  const sk_u32x4 zero = {0u, 0u, 0u, 0u};

  sk_f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
  for (int base = lo + wv * SK_U; base < hi; base += SK_W * SK_U) {
    sk_u32x4 a[SK_U], b[SK_U], xv[SK_U];
    if (base + SK_U <= hi) {  // uniform over the wave
#pragma unroll
      for (int u = 0; u < SK_U; ++u) {
        const long long k0 = (long long)(base + u) << 5;
        a[u] = ldw(wa + k0);
        b[u] = hasB ? ldw(wb + k0) : zero;
        xv[u] = xrow ? *reinterpret_cast<const sk_u32x4*>(xp + k0) : zero;
      }
    } else {
#pragma unroll
      for (int u = 0; u < SK_U; ++u) {
        const bool ok = base + u < hi;
        const long long k0 = (long long)(base + u) << 5;
        a[u] = ok ? ldw(wa + k0) : zero;
        b[u] = ok && hasB ? ldw(wb + k0) : zero;
        xv[u] = ok && xrow ? *reinterpret_cast<const sk_u32x4*>(xp + k0) : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      accA = mfma(a[u], xv[u], accA);
      accB = mfma(b[u], xv[u], accB);
    }
  }

  red[wv][0][lane] = accA;
  red[wv][1][lane] = accB;
  __syncthreads();
  if (wv != 0) return;
  sk_f32x4 ta = red[0][0][lane], tb = red[0][1][lane];
#pragma unroll
  for (int i = 1; i < SK_W; ++i) {  // wave order
    ta += red[i][0][lane];
    tb += red[i][1][lane];
  }
  if (!xrow) return;  // rows m >= M: nothing is written
  const int m = r16, c = kq * 4;
  if (ws) {  // fp32 partial tile of this split, [n_splits][M][N]
    float* p = ws + ((long long)blockIdx.y * M + m) * N;
    *reinterpret_cast<sk_f32x4*>(p + nA + c) = ta;
    if (hasB) *reinterpret_cast<sk_f32x4*>(p + nB + c) = tb;
  } else if (EPI == EPI_SWIGLU) {
    store4_swiglu((uint16_t*)out, (long long)m * ldc + nA + c, ta, tb);
  } else {
    store4(out, out_f32, (long long)m * ldc + nA + c, ta);
    if (hasB) store4(out, out_f32, (long long)m * ldc + nB + c, tb);
  }
}

// The splits of ws [n_splits][M][N] in split order, then the epilogue; one
// thread per four output columns of a row.
template <int EPI>
__global__ __launch_bounds__(SK_T) void k_gemm_skinny_reduce(const float* __restrict__ ws, void* out, long long ldc,
                                                             int out_f32, int M, int N, int n_splits) {
  const int cols = EPI == EPI_SWIGLU ? N >> 1 : N;
  const int q = cols >> 2;
  const int i = blockIdx.x * SK_T + threadIdx.x;
  if (i >= M * q) return;
  const int m = i / q, c = (i - m * q) * 4;
  const long long plane = (long long)M * N;
  const float* p = ws + (long long)m * N + c;
  sk_f32x4 g = *reinterpret_cast<const sk_f32x4*>(p), u = {0.f, 0.f, 0.f, 0.f};
  if (EPI == EPI_SWIGLU) u = *reinterpret_cast<const sk_f32x4*>(p + cols);
  for (int s = 1; s < n_splits; ++s) {
    g += *reinterpret_cast<const sk_f32x4*>(p + s * plane);
    if (EPI == EPI_SWIGLU) u += *reinterpret_cast<const sk_f32x4*>(p + s * plane + cols);
  }
  if (EPI == EPI_SWIGLU)
    store4_swiglu((uint16_t*)out, (long long)m * ldc + c, g, u);
  else
    store4(out, out_f32, (long long)m * ldc + c, g);
}

}  // namespace

#pragma clang attribute pop

#define PTO_API extern "C" __attribute__((visibility("default")))

// The shape rules alone (contiguous operands): 1 <= M <= 16, N % 16 == 0
// (N % 32 == 0 for swiglu: F % 16 == 0), K % 32 == 0.
PTO_API int pto_gemm_skinny_supported(int epilogue, long long M, long long N, long long K) {
  if (epilogue != EPI_PLAIN && epilogue != EPI_SWIGLU) return 0;
  if (M < 1 || M > 16 || N < 16 || K < 32 || K % 32 || K > (1LL << 30)) return 0;
  if (N % (epilogue == EPI_SWIGLU ? 32 : 16) || N > (1LL << 24)) return 0;
  return 1;
}

// Default K split across workgroups, a function of (N, K) alone: enough
// workgroups for two per compute unit of a 256-CU device, while a split keeps
// at least 16 steps (4 per wave).
PTO_API int pto_gemm_skinny_splits(long long N, long long K) {
  if (N < 16 || K < 32) return 1;
  const long long groups = (N + 31) / 32, steps = K / 32;
  long long ns = (512 + groups - 1) / groups;
  if (ns > steps / 16) ns = steps / 16;
  if (ns > 16) ns = 16;
  return ns < 1 ? 1 : (int)ns;
}

// Bytes of fp32 partials a call needs (0 for n_splits == 1).
PTO_API long long pto_gemm_skinny_workspace(long long M, long long N, int n_splits) {
  if (M < 1 || N < 1 || n_splits < 1) return -1;
  return n_splits == 1 ? 0 : (long long)n_splits * M * N * 4;
}

// x bf16 [M][K] (row stride lda), w bf16 [N][K] (ldb), out [M][N] bf16 or
// fp32 (out_f32), or bf16 [M][N/2] = silu(gate) * up for epilogue 1 (w =
// [gate rows; up rows]); strides in elements.  ws: ws_bytes of device memory
// for the fp32 partials when n_splits > 1 (pto_gemm_skinny_workspace).
// Returns -1, having launched nothing, on anything outside the rules.
PTO_API int pto_gemm_skinny(const void* x, long long lda, const void* w, long long ldb, void* out, long long ldc,
                            int out_f32, int epilogue, int M, int N, int K, int n_splits, void* ws,
                            long long ws_bytes, hipStream_t s) {
  if (!pto_gemm_skinny_supported(epilogue, M, N, K)) return -1;
  const int cols = epilogue == EPI_SWIGLU ? N / 2 : N;
  if (epilogue == EPI_SWIGLU && out_f32) return -1;
  if (lda < K || ldb < K || ldc < cols || lda % 8 || ldb % 8 || ldc % 8) return -1;
  if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)out)) & 15) return -1;
  if (n_splits < 1 || n_splits > SK_MAX_SPLITS) return -1;
  float* part = nullptr;
  if (n_splits > 1) {
    if (!ws || (((uintptr_t)ws) & 15) || ws_bytes < pto_gemm_skinny_workspace(M, N, n_splits)) return -1;
    part = (float*)ws;
  }
  const int steps = K / 32;
  const int per = (steps + n_splits - 1) / n_splits;
  const dim3 grid(epilogue == EPI_SWIGLU ? N / 32 : (N + 31) / 32, n_splits);
  const dim3 rgrid((unsigned)((M * (cols / 4) + SK_T - 1) / SK_T));
  if (epilogue == EPI_SWIGLU) {
    hipLaunchKernelGGL(k_gemm_skinny<EPI_SWIGLU>, grid, dim3(SK_T), 0, s, (const uint16_t*)x, lda, (const uint16_t*)w,
                       ldb, out, ldc, 0, part, M, N, K, per);
    if (part)
      hipLaunchKernelGGL(k_gemm_skinny_reduce<EPI_SWIGLU>, rgrid, dim3(SK_T), 0, s, part, out, ldc, 0, M, N, n_splits);
  } else {
    hipLaunchKernelGGL(k_gemm_skinny<EPI_PLAIN>, grid, dim3(SK_T), 0, s, (const uint16_t*)x, lda, (const uint16_t*)w,
                       ldb, out, ldc, out_f32, part, M, N, K, per);
    if (part)
      hipLaunchKernelGGL(k_gemm_skinny_reduce<EPI_PLAIN>, rgrid, dim3(SK_T), 0, s, part, out, ldc, out_f32, M, N,
                         n_splits);
  }
  return (int)hipGetLastError();
}
