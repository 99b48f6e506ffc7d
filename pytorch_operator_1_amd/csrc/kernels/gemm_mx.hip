// Weight-only MX (OCP microscaling) GEMM for any row count: the linear layers
// of a model that holds its weights in packed form only (ops/gemm.py mx_nt,
// linear_mx; models/llama.py Llama.quantize_weights(keep_bf16=False)):
//
//     y[M,N] = x[M,K] . dequant(Wq)[N,K]^T      M >= 1, x bf16, fp32 sums,
//
// Wq exactly as gemm_skinny_mx.hip reads it and k_quant_mx writes it: MXFP4
// (e2m1, element 2i in the low nibble of byte i) uint8 [N][K/2] or MXFP8
// (e4m3fn) uint8 [N][K], one E8M0 scale byte per 32 consecutive K elements of
// a row, uint8 [N][K/32].  No repacked copy exists.  Dequantisation to bf16 is
// exact, so the product is the bf16 product of the quantised model.
//
//   * Work split.  A workgroup (4 waves) owns TM rows of x (a template
//     parameter: 32 for M <= 32, else 64, chosen from M alone; a 128-row
//     instance -- 128 KB of LDS, one workgroup per compute unit -- measured 25
//     to 45 % slower than two 64-row tiles at every M >= 128,
//     profiles/gemm_mx_rows.md, and is not built) and 128 weight rows, and
//     walks one K range.
//     Its waves split N -- 32 weight rows each -- and share the x tile, so
//     every weight element is loaded and unpacked once per workgroup.  With
//     SwiGLU a wave's 32 rows are 16 gate rows n.. and their up rows F + n..
//     (a workgroup then spans 64 gate rows).  blockIdx.x walks the M tiles, so
//     the workgroups that read the same weight rows are dispatched together.
//   * v_mfma_f32_32x32x16_bf16, the wave's 32 weight rows the A operand, 32
//     rows of x the B operand: lane (r = l%32, h = l/32) supplies 8 K elements
//     of weight row r and of x row r.  K is permuted inside a group of 256
//     elements (8 MX blocks): lane (r, h) owns the blocks 4h .. 4h+3 of its
//     weight row -- 64 contiguous bytes of fp4 (four 16-byte loads), 128 of
//     fp8, and ONE aligned 4-byte load of scales; a wave's loads of a group
//     cover 128 (256) contiguous bytes of each of 32 rows, whole cache lines.
//     MFMA c (0..15) of a group contracts chunk c (8 elements) of both halves'
//     blocks against the x chunks at the same K positions.  Packed weights go
//     global -> registers -> v_cvt_scalef32_pk_bf16_fp4/_fp8 (scale e << 23)
//     -> MFMA operand and never touch LDS; one unpacked chunk feeds TM/32
//     MFMAs.
//   * x goes through LDS in the permuted order.  The x slice of a group (TM x
//     256 bf16) is staged by all 256 threads, double buffered, one barrier per
//     group.  16-byte slot ((mt*16 + c)*2 + h)*32 + j holds row mt*32 + j,
//     K chunk h*16 + c.  A fragment read is one ds_read_b128 at slot
//     (mt*16 + c)*64 + lane: 64 lanes, 1024 contiguous bytes, each quarter
//     wave 256 contiguous bytes = every one of the 64 banks once:
//     conflict-free.  Staging thread (j = tid%32, qq = tid/32) moves the
//     chunks 4qq .. 4qq+3 (64 contiguous bytes) of the rows mt*32 + j; a
//     wave's ds_write_b128 is two runs of 512 contiguous bytes, each quarter
//     wave again 256 contiguous bytes: conflict-free.  LDS: TM * 1024 bytes
//     (32 or 64 KB).
//   * Pipeline: the next group's weights and x are loaded into registers
//     before the current group's MFMAs and x is written to the other buffer
//     after them.
//   * Edges.  Rows m >= M load from row M - 1 and are never stored.  A wave
//     whose rows lie past N (past F with SwiGLU) loads no weights and issues
//     no MFMA (a wave-uniform test) but stages x and meets the barriers.  The
//     last group of a K that is no multiple of 256 has no upper half: its
//     weights and x chunks are zeros and nothing is read past K.
//   * K across workgroups: blockIdx.z = split s takes the groups
//     [s*per, (s+1)*per), per = ceil(groups / n_splits); with n_splits > 1 the
//     fp32 tiles go to ws[s][m][n] (the caller's workspace) and a second small
//     launch adds them in split order.  No atomics, counters, allocation or
//     sync: the pair captures into a graph.
//
// Bits: output (m, n) is a function of x[m], row n of the quantised weight, K
// and n_splits alone: the group-to-split map looks at K only, one wave sums an
// element over its groups and MFMAs in order, an MFMA column (a row of x) does
// not depend on the others, and every TM runs the same MFMA sequence.  SwiGLU
// is k_swiglu_fwd's arithmetic on the bf16-rounded gate and up, so bitwise
// ops.llm.swiglu of the plain bf16 result.
#include <hip/hip_runtime.h>
#include <stdint.h>

// packed fp32 VALU forms are kept out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

typedef __bf16 gx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gx_bf16x2 __attribute__((ext_vector_type(2)));
typedef float gx_f32x16 __attribute__((ext_vector_type(16)));
typedef float gx_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned gx_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned gx_u32x2 __attribute__((ext_vector_type(2)));

constexpr int GX_T = 256;      // threads per workgroup
constexpr int GX_GROUP = 256;  // K elements of a group: 8 MX blocks, 4 per lane half
constexpr int GX_MAX_SPLITS = 64;

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

// Four consecutive columns of one output row.
__device__ __forceinline__ void store4(void* out, int out_f32, long long idx, gx_f32x4 v) {
  if (out_f32) {
    *reinterpret_cast<gx_f32x4*>((float*)out + idx) = v;
  } else {
    gx_u32x2 p;
    p.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
    p.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
    *reinterpret_cast<gx_u32x2*>((uint16_t*)out + idx) = p;
  }
}
__device__ __forceinline__ void store4_swiglu(uint16_t* out, long long idx, gx_f32x4 g, gx_f32x4 u) {
  gx_u32x2 p;
  p.x = (uint32_t)swiglu1(g.x, u.x) | ((uint32_t)swiglu1(g.y, u.y) << 16);
  p.y = (uint32_t)swiglu1(g.z, u.z) | ((uint32_t)swiglu1(g.w, u.w) << 16);
  *reinterpret_cast<gx_u32x2*>(out + idx) = p;
}
__device__ __forceinline__ gx_f32x4 quad(const gx_f32x16& a, int b) {
  return gx_f32x4{a[4 * b], a[4 * b + 1], a[4 * b + 2], a[4 * b + 3]};
}

// ---------------------------------------------------------------- weights of one lane, one group
// 4 blocks of one row: 4 (fp4) or 8 (fp8) 16-byte vectors and the 4 scale bytes.
template <int FMT>
struct WRegs {
  static constexpr int NV = FMT == FMT_FP4 ? 4 : 8;
  gx_u32x4 q[NV];
  uint32_t sc;
};

// dp / sp: the lane's row and half, group 0.  !ok (an idle wave, or the half
// lies past K in the last group): zeros, nothing is read.
template <int FMT>
__device__ __forceinline__ void load_w(WRegs<FMT>& r, const uint8_t* dp, const uint8_t* sp, long long g, bool ok) {
  constexpr int NV = WRegs<FMT>::NV;
  const gx_u32x4* p = reinterpret_cast<const gx_u32x4*>(dp + g * (NV * 32));
#pragma unroll
  for (int i = 0; i < NV; ++i) r.q[i] = ok ? p[i] : gx_u32x4{0u, 0u, 0u, 0u};
  r.sc = ok ? *reinterpret_cast<const uint32_t*>(sp + g * 8) : 0x7f7f7f7fu;
}

__device__ __forceinline__ uint32_t pk(gx_bf16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// Chunk j (8 elements) of block u as the bf16 MFMA operand, scaled by s.
template <int FMT>
__device__ __forceinline__ gx_bf16x8 unpack(const WRegs<FMT>& r, int u, int j, float s) {
  gx_u32x4 o;
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
  return __builtin_bit_cast(gx_bf16x8, o);
}

// ---------------------------------------------------------------- x staging
// Thread (j = tid%32, qq = tid/32) moves the chunks q = 4qq + i (i = 0..3) of
// the rows mt*32 + j of the tile: 16 bytes each.  xp[mt]: that row (clamped
// to M - 1), K = 0.
template <int MT>
struct XRegs {
  gx_u32x4 v[MT][4];
};
template <int MT>
__device__ __forceinline__ void load_x(XRegs<MT>& r, const uint16_t* const* xp, long long g, int qq, int K) {
  const long long k = g * GX_GROUP + qq * 32;  // the four chunks lie in one half: all below K or none
  const bool ok = k < K;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      r.v[mt][i] = ok ? *reinterpret_cast<const gx_u32x4*>(xp[mt] + k + i * 8) : gx_u32x4{0u, 0u, 0u, 0u};
}
template <int MT>
__device__ __forceinline__ void store_x(gx_u32x4* buf, const XRegs<MT>& r, int j, int qq) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = qq * 4 + i;
      buf[((mt * 16 + (q & 15)) * 2 + (q >> 4)) * 32 + j] = r.v[mt][i];
    }
}

// Grid (M tiles of TM rows, spans of 128 weight rows -- 64 gate rows with
// SwiGLU --, n_splits), 256 threads, TM * 1024 bytes of dynamic LDS.
template <int FMT, int EPI, int TM>
__global__ __launch_bounds__(GX_T) void k_gemm_mx(const uint16_t* __restrict__ x, long long lda,
                                                  const uint8_t* __restrict__ data,
                                                  const uint8_t* __restrict__ scales, void* out, long long ldc,
                                                  int out_f32, float* __restrict__ ws, int M, int N, int K, int per) {
  constexpr int MT = TM / 32;
  constexpr int SLOTS = TM * 32;  // 16-byte slots of one staged x slice
  extern __shared__ __attribute__((aligned(16))) unsigned char gx_smem[];
  gx_u32x4* xs = reinterpret_cast<gx_u32x4*>(gx_smem);  // [2][SLOTS]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const int F = N >> 1;
  // the wave's weight rows; has is uniform over the wave
  const int n0 = EPI == EPI_SWIGLU ? blockIdx.y * 64 + wv * 16 : blockIdx.y * 128 + wv * 32;
  const bool has = EPI == EPI_SWIGLU ? n0 < F : n0 < N;
  int wrow = 0;
  if (has) wrow = EPI == EPI_SWIGLU ? (r32 < 16 ? n0 + r32 : F + n0 + r32 - 16) : n0 + r32;
  const int m0 = blockIdx.x * TM;
  const int groups = (K + GX_GROUP - 1) / GX_GROUP;
  const int lo = blockIdx.z * per;
  const int hi = lo + per < groups ? lo + per : groups;

  constexpr int ROWB = FMT == FMT_FP4 ? 2 : 1;  // K elements per data byte
  const uint8_t* dp = data + (long long)wrow * (K / ROWB) + h * (128 / ROWB);
  const uint8_t* sp = scales + (long long)wrow * (K >> 5) + h * 4;

  const int xj = tid & 31, xq = tid >> 5;
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 32 + xj;
    xp[mt] = x + (long long)(m < M ? m : M - 1) * lda;
  }

  WRegs<FMT> cw, nw;
  XRegs<MT> xr;
  if (lo < hi) {
    load_w<FMT>(cw, dp, sp, lo, has && (long long)lo * GX_GROUP + h * 128 < K);
    load_x<MT>(xr, xp, lo, xq, K);
    store_x<MT>(xs, xr, xj, xq);
  }
  __syncthreads();

  gx_f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

  for (int g = lo; g < hi; ++g) {
    const int b = (g - lo) & 1;
    const bool more = g + 1 < hi;  // uniform over the workgroup
    if (more) {
      load_w<FMT>(nw, dp, sp, g + 1, has && (long long)(g + 1) * GX_GROUP + h * 128 < K);
      load_x<MT>(xr, xp, g + 1, xq, K);
    }
    if (has) {
      const gx_u32x4* xl = xs + b * SLOTS + lane;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float s = __uint_as_float(((cw.sc >> (8 * u)) & 255u) << 23);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const gx_bf16x8 a = unpack<FMT>(cw, u, j, s);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const gx_bf16x8 xv = __builtin_bit_cast(gx_bf16x8, xl[(mt * 16 + u * 4 + j) * 64]);
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xv, acc[mt], 0, 0, 0);
          }
        }
      }
    }
    if (more) {
      // xs[b ^ 1] was last read before the barrier that ended group g - 1
      store_x<MT>(xs + (b ^ 1) * SLOTS, xr, xj, xq);
      cw = nw;
    }
    __syncthreads();
  }

  if (!has) return;
  // acc[mt][4*b + i] is tile row 8*b + 4*h + i (a weight row), column r32 (row m0 + mt*32 + r32 of x)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 32 + r32;
    if (m >= M) continue;  // rows m >= M: nothing is written
    if (EPI == EPI_SWIGLU) {
#pragma unroll
      for (int bq = 0; bq < 2; ++bq) {  // tile rows 0..15 the gate, 16..31 its up rows
        const int c = n0 + 8 * bq + 4 * h;
        if (ws) {
          float* p = ws + ((long long)blockIdx.z * M + m) * N;
          *reinterpret_cast<gx_f32x4*>(p + c) = quad(acc[mt], bq);
          *reinterpret_cast<gx_f32x4*>(p + F + c) = quad(acc[mt], bq + 2);
        } else {
          store4_swiglu((uint16_t*)out, (long long)m * ldc + c, quad(acc[mt], bq), quad(acc[mt], bq + 2));
        }
      }
    } else {
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) {
        const int c = n0 + 8 * bq + 4 * h;
        if (ws)
          *reinterpret_cast<gx_f32x4*>(ws + ((long long)blockIdx.z * M + m) * N + c) = quad(acc[mt], bq);
        else
          store4(out, out_f32, (long long)m * ldc + c, quad(acc[mt], bq));
      }
    }
  }
}

// The splits of ws [n_splits][M][N] in split order, then the epilogue; one
// thread per four output columns of a row.
template <int EPI>
__global__ __launch_bounds__(GX_T) void k_gemm_mx_reduce(const float* __restrict__ ws, void* out, long long ldc,
                                                         int out_f32, int M, int N, int n_splits) {
  const int cols = EPI == EPI_SWIGLU ? N >> 1 : N;
  const long long q = cols >> 2;
  const long long i = (long long)blockIdx.x * GX_T + threadIdx.x;
  if (i >= M * q) return;
  const long long m = i / q;
  const int c = (int)(i - m * q) * 4;
  const long long plane = (long long)M * N;
  const float* p = ws + m * N + c;
  gx_f32x4 g = *reinterpret_cast<const gx_f32x4*>(p), u = {0.f, 0.f, 0.f, 0.f};
  if (EPI == EPI_SWIGLU) u = *reinterpret_cast<const gx_f32x4*>(p + cols);
  for (int s = 1; s < n_splits; ++s) {
    g += *reinterpret_cast<const gx_f32x4*>(p + s * plane);
    if (EPI == EPI_SWIGLU) u += *reinterpret_cast<const gx_f32x4*>(p + s * plane + cols);
  }
  if (EPI == EPI_SWIGLU)
    store4_swiglu((uint16_t*)out, m * ldc + c, g, u);
  else
    store4(out, out_f32, m * ldc + c, g);
}

// The M tile: a function of M alone.
inline int tile_rows(long long M) { return M <= 32 ? 32 : 64; }

template <int FMT, int EPI, int TM>
int launch(dim3 grid, hipStream_t s, const uint16_t* x, long long lda, const uint8_t* data, const uint8_t* scales,
           void* out, long long ldc, int out_f32, float* ws, int M, int N, int K, int per) {
  constexpr int LDS = TM * 1024;
  static const int attr =
      (int)hipFuncSetAttribute((const void*)k_gemm_mx<FMT, EPI, TM>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  if (attr != 0) return attr;
  hipLaunchKernelGGL((k_gemm_mx<FMT, EPI, TM>), grid, dim3(GX_T), LDS, s, x, lda, data, scales, out, ldc, out_f32, ws,
                     M, N, K, per);
  return 0;
}

template <int FMT, int EPI>
int launch_tm(int tm, dim3 grid, hipStream_t s, const uint16_t* x, long long lda, const uint8_t* data,
              const uint8_t* scales, void* out, long long ldc, int out_f32, float* ws, int M, int N, int K, int per) {
  if (tm == 32) return launch<FMT, EPI, 32>(grid, s, x, lda, data, scales, out, ldc, out_f32, ws, M, N, K, per);
  return launch<FMT, EPI, 64>(grid, s, x, lda, data, scales, out, ldc, out_f32, ws, M, N, K, per);
}

}  // namespace

#pragma clang attribute pop

#define PTO_API extern "C" __attribute__((visibility("default")))

// The shape rules alone (contiguous operands): fmt 0 (mxfp4) or 1 (mxfp8),
// M >= 1, N % 32 == 0 (N % 64 == 0 for swiglu), K % 128 == 0.
PTO_API int pto_gemm_mx_supported(int epilogue, int fmt, long long M, long long N, long long K) {
  if (epilogue != EPI_PLAIN && epilogue != EPI_SWIGLU) return 0;
  if (fmt != FMT_FP4 && fmt != FMT_FP8) return 0;
  if (M < 1 || M > (1LL << 24) || N < 32 || K < 128 || K % 128 || K > (1LL << 30)) return 0;
  if (N % (epilogue == EPI_SWIGLU ? 64 : 32) || N > (1LL << 22) || M * N > (1LL << 33)) return 0;
  return 1;
}

// Default K split across workgroups, a function of the shape alone: enough
// workgroups for two per compute unit of a 256-CU device while a split keeps
// at least two groups, so that its register prefetch has something to hide.
PTO_API int pto_gemm_mx_splits(long long M, long long N, long long K, int fmt) {
  (void)fmt;
  if (M < 1 || N < 32 || K < 128) return 1;
  const long long tm = tile_rows(M);
  const long long wgs = ((M + tm - 1) / tm) * ((N + 127) / 128), groups = (K + GX_GROUP - 1) / GX_GROUP;
  long long ns = 512 / wgs;
  if (ns > groups / 2) ns = groups / 2;
  if (ns > 16) ns = 16;
  return ns < 1 ? 1 : (int)ns;
}

// Bytes of fp32 partials a call needs (0 for n_splits == 1).
PTO_API long long pto_gemm_mx_workspace(long long M, long long N, int n_splits) {
  if (M < 1 || N < 1 || n_splits < 1) return -1;
  return n_splits == 1 ? 0 : (long long)n_splits * M * N * 4;
}

// x bf16 [M][K] (row stride lda elements), data / scales the contiguous MX
// weight [N][K] in format fmt, out [M][N] bf16 or fp32 (out_f32; row stride
// ldc), or bf16 [M][N/2] = silu(gate) * up for epilogue 1 (rows [gate; up]).
// ws: ws_bytes of device memory for the fp32 partials when n_splits > 1.
// Returns -1, having launched nothing, on anything outside the rules.
PTO_API int pto_gemm_mx(const void* x, long long lda, const void* data, const void* scales, void* out, long long ldc,
                        int out_f32, int epilogue, int fmt, long long M, long long N, long long K, int n_splits,
                        void* ws, long long ws_bytes, hipStream_t s) {
  if (!pto_gemm_mx_supported(epilogue, fmt, M, N, K)) return -1;
  const long long cols = epilogue == EPI_SWIGLU ? N / 2 : N;
  if (epilogue == EPI_SWIGLU && out_f32) return -1;
  if (lda < K || ldc < cols || lda % 8 || ldc % 8) return -1;
  if (!x || !data || !scales || !out) return -1;
  if ((((uintptr_t)x) | ((uintptr_t)data) | ((uintptr_t)scales) | ((uintptr_t)out)) & 15) return -1;
  if (n_splits < 1 || n_splits > GX_MAX_SPLITS) return -1;
  float* part = nullptr;
  if (n_splits > 1) {
    if (!ws || (((uintptr_t)ws) & 15) || ws_bytes < pto_gemm_mx_workspace(M, N, n_splits)) return -1;
    part = (float*)ws;
  }
  const int groups = (int)((K + GX_GROUP - 1) / GX_GROUP);
  const int per = (groups + n_splits - 1) / n_splits;
  const int tm = tile_rows(M);
  const dim3 grid((unsigned)((M + tm - 1) / tm), (unsigned)(epilogue == EPI_SWIGLU ? (N / 2 + 63) / 64 : (N + 127) / 128),
                  (unsigned)n_splits);
  const dim3 rgrid((unsigned)((M * (cols / 4) + GX_T - 1) / GX_T));
  const uint16_t* xp = (const uint16_t*)x;
  const uint8_t *dp = (const uint8_t*)data, *sp = (const uint8_t*)scales;
  int rc;
#define GX_LAUNCH(FMT, EPI, F32) \
  rc = launch_tm<FMT, EPI>(tm, grid, s, xp, lda, dp, sp, out, ldc, F32, part, (int)M, (int)N, (int)K, per)
  if (epilogue == EPI_SWIGLU) {
    if (fmt == FMT_FP4)
      GX_LAUNCH(FMT_FP4, EPI_SWIGLU, 0);
    else
      GX_LAUNCH(FMT_FP8, EPI_SWIGLU, 0);
    if (rc != 0) return rc;
    if (part)
      hipLaunchKernelGGL(k_gemm_mx_reduce<EPI_SWIGLU>, rgrid, dim3(GX_T), 0, s, part, out, ldc, 0, (int)M, (int)N,
                         n_splits);
  } else {
    if (fmt == FMT_FP4)
      GX_LAUNCH(FMT_FP4, EPI_PLAIN, out_f32);
    else
      GX_LAUNCH(FMT_FP8, EPI_PLAIN, out_f32);
    if (rc != 0) return rc;
    if (part)
      hipLaunchKernelGGL(k_gemm_mx_reduce<EPI_PLAIN>, rgrid, dim3(GX_T), 0, s, part, out, ldc, out_f32, (int)M, (int)N,
                         n_splits);
  }
#undef GX_LAUNCH
  return (int)hipGetLastError();
}
