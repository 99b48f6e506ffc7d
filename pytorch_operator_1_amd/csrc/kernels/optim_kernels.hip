// Multi-tensor AdamW for the large-model configs (ResNet-50 / Llama-3-8B
// DDP, BASELINE configs 3-4), one launch for every parameter tensor.
//
// Mixed precision layout (sized for 288 GB HBM per MI355X): model params
// and grads in bf16 (what the forward/backward and the RCCL bucket
// all-reduce touch: 2 + 2 bytes/param), fp32 master weights + fp32 Adam
// moments held only by the optimizer (12 bytes/param).  Llama-3-8B:
// 8.03e9 x 16 B = 128 GB per GPU before activations.
//
// The op is HBM-bound (per param: read 2+4+4+4, write 2+4+4+4 bytes), so
// every lane moves 8 elements per step: 16-byte bf16 loads/stores and
// 2 x 16-byte fp32 accesses per state tensor (Guideline 13).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mfma_f32.h"

struct AdamTensor {
  void* p;         // param: bf16 (mixed) or fp32
  void* g;         // grad: bf16 (mixed) or fp32
  float* master;   // fp32 master weights (mixed only; nullptr for fp32 params)
  float* m;
  float* v;
  long long n;
};

// record of k_grad_accum_multi (micro-batch gradient accumulation, below)
struct AccumTensor {
  const void* g;  // gradient of this micro-batch: bf16 or fp32; nullptr = none
  float* acc;     // fp32 running sum
  void* out;      // FOLD only: destination in the gradient's dtype
  long long n;
};

namespace {

constexpr int ADAM_CHUNK = 256 * 8;  // elements per block (8 per thread)

__device__ __forceinline__ float bf2f(uint16_t x) { return __uint_as_float(((uint32_t)x) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {  // round-to-nearest-even
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);  // inf/nan
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct AdamHyper {
  float lr, beta1, beta2, eps, wd, bc1, bc2, gscale;
};

__device__ __forceinline__ void adam_elem(float& w, float g, float& m, float& v, const AdamHyper& h) {
  g *= h.gscale;
  m = h.beta1 * m + (1.f - h.beta1) * g;
  v = h.beta2 * v + (1.f - h.beta2) * g * g;
  const float mhat = m / h.bc1, vhat = v / h.bc2;
  w = w * (1.f - h.lr * h.wd) - h.lr * mhat / (sqrtf(vhat) + h.eps);  // decoupled decay (AdamW)
}

// CLIP: each gradient is multiplied by *gscale_ptr (the global-norm clip
// coefficient of k_grad_norm_finalize, read once per thread) on its way into
// adam_elem, so the effective scale is gscale * coef.  Two things are
// deliberate (profiles/grad_clip.md):
//  * a template parameter, not a test of the pointer: with the test in the
//    kernel hipcc contracted adam_elem's multiply-adds differently (another
//    sequence of fp instructions, so other roundings, for callers that pass
//    no pointer) and the launch was 0.6-1.0 % slower.  The plain instance
//    keeps the instructions it had.
//  * the coefficient goes onto the gradient, not into h.gscale: h.gscale
//    stays the kernel argument it is in the plain instance, adam_elem
//    compiles to the same operations in both, and a coefficient of exactly
//    1.0 (max_norm = inf) gives bit for bit the unclipped update.
template <bool MIXED, bool CLIP>
__global__ __launch_bounds__(256) void k_adamw_multi(const AdamTensor* __restrict__ ts,
                                                     const int* __restrict__ block_start, int ntensors,
                                                     const float* __restrict__ lr_ptr, AdamHyper h,
                                                     int zero_grad, const float* __restrict__ gscale_ptr) {
  int lo = 0, hi = ntensors - 1;
  const int bid = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_start[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  const AdamTensor t = ts[lo];
  if (lr_ptr) h.lr = *lr_ptr;
  const float coef = CLIP ? *gscale_ptr : 1.f;
  const long long i0 = (long long)(bid - block_start[lo]) * ADAM_CHUNK + (long long)threadIdx.x * 8;
  if (i0 >= t.n) return;
  const bool full = i0 + 8 <= t.n;
  if (MIXED) {
    uint16_t* pb = reinterpret_cast<uint16_t*>(t.p);
    uint16_t* gb = reinterpret_cast<uint16_t*>(t.g);
    const bool vec = full && ((((uintptr_t)(pb + i0)) | ((uintptr_t)(gb + i0)) | ((uintptr_t)(t.master + i0)) |
                               ((uintptr_t)(t.m + i0)) | ((uintptr_t)(t.v + i0))) & 15) == 0;
    if (vec) {
      const uint4 gv = *reinterpret_cast<const uint4*>(gb + i0);
      float4 w0 = reinterpret_cast<float4*>(t.master + i0)[0], w1 = reinterpret_cast<float4*>(t.master + i0)[1];
      float4 m0 = reinterpret_cast<float4*>(t.m + i0)[0], m1 = reinterpret_cast<float4*>(t.m + i0)[1];
      float4 v0 = reinterpret_cast<float4*>(t.v + i0)[0], v1 = reinterpret_cast<float4*>(t.v + i0)[1];
      const uint16_t* gs = reinterpret_cast<const uint16_t*>(&gv);
      float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
      float m[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      uint16_t out[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        adam_elem(w[j], CLIP ? bf2f(gs[j]) * coef : bf2f(gs[j]), m[j], v[j], h);
        out[j] = f2bf(w[j]);
      }
      reinterpret_cast<float4*>(t.master + i0)[0] = float4{w[0], w[1], w[2], w[3]};
      reinterpret_cast<float4*>(t.master + i0)[1] = float4{w[4], w[5], w[6], w[7]};
      reinterpret_cast<float4*>(t.m + i0)[0] = float4{m[0], m[1], m[2], m[3]};
      reinterpret_cast<float4*>(t.m + i0)[1] = float4{m[4], m[5], m[6], m[7]};
      reinterpret_cast<float4*>(t.v + i0)[0] = float4{v[0], v[1], v[2], v[3]};
      reinterpret_cast<float4*>(t.v + i0)[1] = float4{v[4], v[5], v[6], v[7]};
      *reinterpret_cast<uint4*>(pb + i0) = *reinterpret_cast<const uint4*>(out);
      if (zero_grad) *reinterpret_cast<uint4*>(gb + i0) = uint4{0, 0, 0, 0};
    } else {
      for (long long e = i0; e < i0 + 8 && e < t.n; ++e) {
        float w = t.master[e], m = t.m[e], v = t.v[e];
        adam_elem(w, CLIP ? bf2f(gb[e]) * coef : bf2f(gb[e]), m, v, h);
        t.master[e] = w; t.m[e] = m; t.v[e] = v;
        pb[e] = f2bf(w);
        if (zero_grad) gb[e] = 0;
      }
    }
  } else {
    float* p = reinterpret_cast<float*>(t.p);
    float* g = reinterpret_cast<float*>(t.g);
    for (long long e = i0; e < i0 + 8 && e < t.n; ++e) {
      float w = p[e], m = t.m[e], v = t.v[e];
      adam_elem(w, CLIP ? g[e] * coef : g[e], m, v, h);
      p[e] = w; t.m[e] = m; t.v[e] = v;
      if (zero_grad) g[e] = 0.f;
    }
  }
}

// ---- global gradient norm (clip_grad_norm_ without a host sync) ----------
//
// Stage 1, k_grad_sqnorm_multi: sum of squares over every gradient of a
// launch table (AdamTensor or SgdTensor records: the gradient pointer is the
// second field, the element count the last).  The gradients are cut into
// chunks of SQN_CHUNK elements (8 per thread, k_adamw_multi's access
// pattern); chunk_start[t] is the first chunk of tensor t and
// chunk_start[ntensors] the total.  A workgroup owns SQN_CPB consecutive
// chunks, whatever tensors they belong to, and writes ONE partial.
//
// Stage 2, k_grad_norm_finalize: one workgroup sums the partials and writes
// {total_norm, coef}; the optimizer kernels multiply their gradient scale
// by coef, read from device memory.
//
// Every replica of a DDP job must derive the same coefficient from the same
// (all-reduced) gradients, so the order of every addition is fixed by the
// table alone: no atomics, no dependence on which block finishes first.
//   thread: 8 accumulators (element j of its 8), one fma per chunk in chunk
//           order, then ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7));
//   wave:   wave_sum (6 exchange steps);   block: waves 0..3 in order.
constexpr int SQN_CHUNK = 256 * 8;  // elements per chunk
constexpr int SQN_CPB = 32;         // chunks per workgroup (128 KB of bf16): 8 B params -> 122k partials, 0.5 MB
constexpr int FIN_THREADS = 1024;   // stage 2 workgroup

template <bool BF16>
__device__ __forceinline__ void sqn_chunk(const void* g, long long n, long long i0, float (&acc)[8]) {
  if (i0 >= n) return;
  if (BF16) {
    const uint16_t* gb = reinterpret_cast<const uint16_t*>(g);
    if (i0 + 8 <= n && (((uintptr_t)(gb + i0)) & 15) == 0) {
      const uint4 gv = *reinterpret_cast<const uint4*>(gb + i0);
      const uint16_t* gs = reinterpret_cast<const uint16_t*>(&gv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = bf2f(gs[j]);
        acc[j] = fmaf(x, x, acc[j]);
      }
    } else {
      for (int j = 0; j < 8 && i0 + j < n; ++j) {
        const float x = bf2f(gb[i0 + j]);
        acc[j] = fmaf(x, x, acc[j]);
      }
    }
  } else {
    const float* gf = reinterpret_cast<const float*>(g);
    if (i0 + 8 <= n && (((uintptr_t)(gf + i0)) & 15) == 0) {
      const float4 a = reinterpret_cast<const float4*>(gf + i0)[0], b = reinterpret_cast<const float4*>(gf + i0)[1];
      const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(x[j], x[j], acc[j]);
    } else {
      for (int j = 0; j < 8 && i0 + j < n; ++j) {
        const float x = gf[i0 + j];
        acc[j] = fmaf(x, x, acc[j]);
      }
    }
  }
}

template <bool BF16>
__global__ __launch_bounds__(256) void k_grad_sqnorm_multi(const char* __restrict__ ts, int stride,
                                                           const int* __restrict__ chunk_start, int ntensors,
                                                           float* __restrict__ partials) {
  const int total = chunk_start[ntensors];
  const int c0 = blockIdx.x * SQN_CPB;
  const int c1 = min(c0 + SQN_CPB, total);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < c1) {
    int lo = 0, hi = ntensors - 1;  // last tensor whose first chunk is <= c0 (empty tensors are skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (chunk_start[mid] <= c0) lo = mid; else hi = mid - 1;
    }
    int t = lo, c = c0;
    while (c < c1) {
      while (chunk_start[t + 1] <= c) ++t;  // c < total = chunk_start[ntensors]: t stays < ntensors
      const char* rec = ts + (size_t)t * stride;
      const void* g = *reinterpret_cast<const void* const*>(rec + sizeof(void*));
      const long long n = *reinterpret_cast<const long long*>(rec + stride - sizeof(long long));
      const int cend = min(c1, chunk_start[t + 1]);
      long long i0 = (long long)(c - chunk_start[t]) * SQN_CHUNK + (long long)threadIdx.x * 8;
      // whole chunks of an aligned tensor: branch-free loads, four chunks in
      // flight per thread (same additions in the same order as sqn_chunk)
      const int cfull = (((uintptr_t)g) & 15) == 0 ? min(cend, chunk_start[t] + (int)(n / SQN_CHUNK)) : c;
      for (; c + 4 <= cfull; c += 4, i0 += 4 * SQN_CHUNK) {
        if (BF16) {
          const uint16_t* gb = reinterpret_cast<const uint16_t*>(g) + i0;
          uint4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const uint4*>(gb + u * SQN_CHUNK);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint16_t* gs = reinterpret_cast<const uint16_t*>(&v[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float x = bf2f(gs[j]);
              acc[j] = fmaf(x, x, acc[j]);
            }
          }
        } else {
          const float* gf = reinterpret_cast<const float*>(g) + i0;
          float4 v[8];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v[2 * u] = reinterpret_cast<const float4*>(gf + u * SQN_CHUNK)[0];
            v[2 * u + 1] = reinterpret_cast<const float4*>(gf + u * SQN_CHUNK)[1];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float x[8] = {v[2 * u].x, v[2 * u].y, v[2 * u].z, v[2 * u].w,
                                v[2 * u + 1].x, v[2 * u + 1].y, v[2 * u + 1].z, v[2 * u + 1].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(x[j], x[j], acc[j]);
          }
        }
      }
      for (; c < cend; ++c, i0 += SQN_CHUNK) sqn_chunk<BF16>(g, n, i0, acc);
    }
  }
  float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  s = wave_sum(s);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// rec[0] = gscale * sqrt(sum)  (norm of the MEAN gradient: the buffers hold the sum over ranks)
// rec[1] = min(1, max_norm / (rec[0] + 1e-6)), NaN kept as torch.clamp(max=1) keeps it
__global__ __launch_bounds__(FIN_THREADS) void k_grad_norm_finalize(const float* __restrict__ partials, int n,
                                                                    float gscale, float max_norm,
                                                                    float* __restrict__ rec) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += FIN_THREADS) s += partials[i];
  s = wave_sum(s);
  __shared__ float ws[FIN_THREADS / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = ws[0];
    for (int w = 1; w < FIN_THREADS / 64; ++w) tot += ws[w];
    const float norm = gscale * sqrtf(tot);
    const float c = max_norm / (norm + 1e-6f);
    rec[0] = norm;
    rec[1] = c > 1.f ? 1.f : c;
  }
}

// ---- micro-batch gradient accumulation in fp32 ---------------------------
//
// One optimizer step over N micro-batches sums their gradients in an fp32
// accumulator per parameter (a bf16 running sum of magnitude 256 no longer
// sees an addend of 1).  One launch per table, k_adamw_multi's layout: a
// record per tensor, block_start[t] the first block of tensor t, ACC_CHUNK
// elements per block, 8 per thread.
//   ACC_INIT  acc = float(g)                 first micro-batch: no zeroing pass
//   ACC_ADD   acc = acc + float(g)           one fp32 add
//   ACC_FOLD  out = cast(acc + float(g))     last micro-batch; acc is NOT written
// cast is f2bf for bf16 gradients, the identity for fp32.  out may be g itself
// (every thread reads its 8 elements before it writes them) or another buffer
// (a bucket slot).  g == nullptr is a parameter without a gradient in this
// micro-batch, g = 0: INIT writes zeros, ADD does nothing, FOLD writes
// cast(acc).  Plain vector stores, no atomics: the result is a pure function
// of the inputs.  Mode and dtype are template parameters for the reason given
// above k_adamw_multi.
constexpr int ACC_CHUNK = 256 * 8;  // elements per block (8 per thread)
enum { ACC_INIT = 0, ACC_ADD = 1, ACC_FOLD = 2 };

template <bool BF16>
__device__ __forceinline__ void acc_load_g(const void* g, long long i0, float (&x)[8]) {
  if (BF16) {
    const uint4 gv = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(g) + i0);
    const uint16_t* gs = reinterpret_cast<const uint16_t*>(&gv);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = bf2f(gs[j]);
  } else {
    const float4* gp = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g) + i0);
    const float4 a = gp[0], b = gp[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  }
}

template <bool BF16, int MODE>
__global__ __launch_bounds__(256) void k_grad_accum_multi(const AccumTensor* __restrict__ ts,
                                                          const int* __restrict__ block_start, int ntensors) {
  int lo = 0, hi = ntensors - 1;
  const int bid = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_start[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  const AccumTensor t = ts[lo];
  const long long i0 = (long long)(bid - block_start[lo]) * ACC_CHUNK + (long long)threadIdx.x * 8;
  if (i0 >= t.n) return;
  const bool has_g = t.g != nullptr;  // uniform over the block
  if (MODE == ACC_ADD && !has_g) return;
  constexpr int GB = BF16 ? 2 : 4;  // bytes per gradient element
  uintptr_t addr = (uintptr_t)(t.acc + i0);
  if (has_g) addr |= (uintptr_t)t.g + (uintptr_t)i0 * GB;
  if (MODE == ACC_FOLD) addr |= (uintptr_t)t.out + (uintptr_t)i0 * GB;
  if (i0 + 8 <= t.n && (addr & 15) == 0) {
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (has_g) acc_load_g<BF16>(t.g, i0, x);
    float4* ap = reinterpret_cast<float4*>(t.acc + i0);
    if (MODE != ACC_INIT) {
      const float4 a = ap[0], b = ap[1];
      const float s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if (has_g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = s[j] + x[j];
      } else {  // FOLD without a gradient: cast(acc), not acc + 0 (keeps -0)
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = s[j];
      }
    }
    if (MODE != ACC_FOLD) {
      ap[0] = float4{x[0], x[1], x[2], x[3]};
      ap[1] = float4{x[4], x[5], x[6], x[7]};
    } else if (BF16) {
      uint16_t o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(x[j]);
      *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(t.out) + i0) = *reinterpret_cast<const uint4*>(o);
    } else {
      float4* op = reinterpret_cast<float4*>(reinterpret_cast<float*>(t.out) + i0);
      op[0] = float4{x[0], x[1], x[2], x[3]};
      op[1] = float4{x[4], x[5], x[6], x[7]};
    }
  } else {
    for (long long e = i0; e < i0 + 8 && e < t.n; ++e) {
      float x = 0.f;
      if (has_g) x = BF16 ? bf2f(reinterpret_cast<const uint16_t*>(t.g)[e]) : reinterpret_cast<const float*>(t.g)[e];
      if (MODE != ACC_INIT) x = has_g ? t.acc[e] + x : t.acc[e];
      if (MODE != ACC_FOLD) t.acc[e] = x;
      else if (BF16) reinterpret_cast<uint16_t*>(t.out)[e] = f2bf(x);
      else reinterpret_cast<float*>(t.out)[e] = x;
    }
  }
}

// bf16 <-> fp32 flat casts (master-weight init, checkpoint export)
__global__ __launch_bounds__(256) void k_bf16_to_f32(const uint16_t* __restrict__ x, float* __restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = bf2f(x[i]);
}

}  // namespace

#define PTO_API extern "C" __attribute__((visibility("default")))

PTO_API int pto_adamw_block_count(long long n) { return (int)((n + ADAM_CHUNK - 1) / ADAM_CHUNK); }

// The reduction's shape, for callers sizing buffers and for the tests' error bound.
PTO_API int pto_grad_sqnorm_chunks(long long n) { return (int)((n + SQN_CHUNK - 1) / SQN_CHUNK); }
PTO_API int pto_grad_sqnorm_blocks(long long chunks) { return (int)((chunks + SQN_CPB - 1) / SQN_CPB); }
PTO_API int pto_grad_sqnorm_chunks_per_block(void) { return SQN_CPB; }
PTO_API int pto_grad_norm_finalize_threads(void) { return FIN_THREADS; }

// pto_adamw_multi with the gradient scale multiplied by *gscale_ptr (device
// memory: the clip coefficient of pto_grad_norm_finalize); nullptr: gscale alone.
PTO_API int pto_adamw_multi_clip(const AdamTensor* ts, const int* block_start, int ntensors, int nblocks, int mixed,
                                 const float* lr_ptr, float lr, float beta1, float beta2, float eps, float wd,
                                 int step, float gscale, const float* gscale_ptr, int zero_grad, hipStream_t s) {
  if (nblocks <= 0) return 0;
  AdamHyper h{lr, beta1, beta2, eps, wd, 1.f - powf(beta1, (float)step), 1.f - powf(beta2, (float)step), gscale};
  auto k = mixed ? (gscale_ptr ? k_adamw_multi<true, true> : k_adamw_multi<true, false>)
                 : (gscale_ptr ? k_adamw_multi<false, true> : k_adamw_multi<false, false>);
  hipLaunchKernelGGL(k, dim3(nblocks), dim3(256), 0, s, ts, block_start, ntensors, lr_ptr, h, zero_grad, gscale_ptr);
  return (int)hipGetLastError();
}

// step = 1-based optimizer step (bias corrections computed here).
PTO_API int pto_adamw_multi(const AdamTensor* ts, const int* block_start, int ntensors, int nblocks, int mixed,
                            const float* lr_ptr, float lr, float beta1, float beta2, float eps, float wd, int step,
                            float gscale, int zero_grad, hipStream_t s) {
  return pto_adamw_multi_clip(ts, block_start, ntensors, nblocks, mixed, lr_ptr, lr, beta1, beta2, eps, wd, step,
                              gscale, nullptr, zero_grad, s);
}

// Stage 1 of the gradient norm.  ts: device table of `stride`-byte records
// (AdamTensor / SgdTensor); chunk_start: ntensors + 1 device ints, prefix of
// pto_grad_sqnorm_chunks(n); partials: nblocks = pto_grad_sqnorm_blocks(total
// chunks) floats, every one of them written.
PTO_API int pto_grad_sqnorm_multi(const void* ts, int stride, const int* chunk_start, int ntensors, int bf16,
                                  float* partials, int nblocks, hipStream_t s) {
  if (nblocks <= 0 || ntensors <= 0) return 0;
  if (stride < (int)(sizeof(void*) * 2 + sizeof(long long))) return (int)hipErrorInvalidValue;
  const char* t = reinterpret_cast<const char*>(ts);
  if (bf16)
    hipLaunchKernelGGL(k_grad_sqnorm_multi<true>, dim3(nblocks), dim3(256), 0, s, t, stride, chunk_start, ntensors,
                       partials);
  else
    hipLaunchKernelGGL(k_grad_sqnorm_multi<false>, dim3(nblocks), dim3(256), 0, s, t, stride, chunk_start, ntensors,
                       partials);
  return (int)hipGetLastError();
}

// Stage 2: rec[0] = gscale * sqrt(sum of the n partials), rec[1] = clip coefficient.
PTO_API int pto_grad_norm_finalize(const float* partials, int n, float gscale, float max_norm, float* rec,
                                   hipStream_t s) {
  hipLaunchKernelGGL(k_grad_norm_finalize, dim3(1), dim3(FIN_THREADS), 0, s, partials, n, gscale, max_norm, rec);
  return (int)hipGetLastError();
}

PTO_API int pto_grad_accum_block_count(long long n) { return (int)((n + ACC_CHUNK - 1) / ACC_CHUNK); }

// fp32 micro-batch accumulation over a device table of AccumTensor records.
// block_start: ntensors device ints, prefix of pto_grad_accum_block_count(n);
// bf16: the gradients' (and FOLD's out) dtype; mode: 0 INIT, 1 ADD, 2 FOLD.
PTO_API int pto_grad_accum_multi(const AccumTensor* ts, const int* block_start, int ntensors, int nblocks, int bf16,
                                 int mode, hipStream_t s) {
  if (mode < ACC_INIT || mode > ACC_FOLD) return (int)hipErrorInvalidValue;
  if (nblocks <= 0 || ntensors <= 0) return 0;
  void (*k)(const AccumTensor*, const int*, int);
  if (bf16)
    k = mode == ACC_INIT ? k_grad_accum_multi<true, ACC_INIT>
      : mode == ACC_ADD  ? k_grad_accum_multi<true, ACC_ADD> : k_grad_accum_multi<true, ACC_FOLD>;
  else
    k = mode == ACC_INIT ? k_grad_accum_multi<false, ACC_INIT>
      : mode == ACC_ADD  ? k_grad_accum_multi<false, ACC_ADD> : k_grad_accum_multi<false, ACC_FOLD>;
  hipLaunchKernelGGL(k, dim3(nblocks), dim3(256), 0, s, ts, block_start, ntensors);
  return (int)hipGetLastError();
}

PTO_API int pto_bf16_to_f32(const void* x, float* y, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_bf16_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const uint16_t*>(x), y, n);
  return (int)hipGetLastError();
}
