// Weight gradient of the 3x3 convolutions (pad 1, stride 1 or 2) as an MFMA
// GEMM over channels-last bf16, C and K independent multiples of 64.
//
// GEMM view: dW[k][r][s][c] = sum_p dy[p][k] * x[n, oh S + r - 1, ow S + s - 1][c],
// p = (n, oh, ow) over the P = N OH OW output pixels; M = K, N = 9 C, and the
// reduction runs over PIXELS.  Both operands are [pixel][channel] in memory,
// i.e. contiguous along the output dimensions and strided along the
// reduction: the case ds_read_b64_tr_b16 exists for.  A lane of
// v_mfma_f32_32x32x16_bf16 needs 8 consecutive reduction elements (pixels) of
// one channel; two transposed reads deliver them from a [pixel][channel] LDS
// image, and every lane supplies the address of its own pixel row, so the
// rows of a block need not be evenly spaced.
//
// Workgroup: 256 threads = 4 waves, one 64 (k) x 64 (c) tile of ALL 9 taps;
// wave (mi, ni) owns the 32 x 32 quadrant of every tap (9 accumulators, 144
// registers).  It walks chunks of output rows ("units" u = n OH + oh; of a
// column range of them where one whole row is too wide).  Per chunk the block
// stages
//   * the dy rows of the chunk's pixels, compact, [pixel][64 k], padded with
//     zero rows to a multiple of 16 pixels;
//   * ONE strip of x: the input rows the chunk's windows touch, each with a
//     zero column on either side, zero rows above / below each image, as
//     [strip pixel][64 c].  A tap is then only a row offset (r WPS + s, WPS
//     the strip's width in pixels) into that image and stride 2 only a row
//     stride, so x is fetched once per chunk, not once per tap;
//   * a table: per dy pixel, the byte offset of its window origin in the strip.
// Padding comes from buffer loads at an out-of-range offset (zeros), as in
// the forward kernel.  No lane is ever masked at a transposed read: the pixel
// loop is wave-uniform and the tile is padded with zero dy rows (their table
// entry is 0, the first three strip rows, always staged; a zero dy row
// times a non-finite x there gives NaN, as the true sum over an x with
// non-finite values does for that input channel in all but contrived cases).
//
// Pipeline: a chunk's operands are loaded into registers (WG_XL + WG_DL
// 16-byte loads per thread) while the previous chunk multiplies, and two
// workgroups share a CU (256 registers each), so the loads of one chunk have
// a whole chunk of MFMA time to arrive.
//
// LDS layout and bank conflicts (bank = (addr / 4) % 64, counted per 32-lane
// half): a half reads 4 pixel rows x 64 contiguous bytes.  dy rows and
// stride-1 x rows are 192 bytes apart: 4 consecutive rows start at 0, 192,
// 128, 64 (mod 256), four disjoint 64-byte bank ranges -- conflict-free at
// any tap offset.  Stride-2 x rows are 160 bytes apart: rows 2q start at 0,
// 64, 128, 192 (mod 256) -- conflict-free.  A 4-pixel block that straddles
// the end of an output row (its x rows jump by the halo) is up to 2-way.
//
// The reduction is split over workgroups: split i sums its chunks into the
// fp32 workspace slot ws[i][K 9 C]; k_conv3x3_wgrad_reduce adds the slots in
// split order.  No atomics: the result is bitwise repeatable, and the split
// count depends on the shape and compile-time constants only.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned wg_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wg_u32x2 __attribute__((ext_vector_type(2)));
typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) wg_s16x4 wg_lds_s16x4;

constexpr int WG_T = 256;         // threads per block
constexpr int WG_DP = 192;        // bytes per staged dy pixel row (128 of data)
constexpr int WG_LDS = 79 * 1024; // LDS budget per workgroup (two per CU)
constexpr int WG_XL = 10;         // 16-byte loads per thread per chunk, x strip: at most 32 WG_XL strip pixels
constexpr int WG_DL = 4;          // the same for dy: at most 32 WG_DL pixels
constexpr int WG_TARGET = 512;    // workgroups aimed for (tiles x splits): one resident wave of two per CU on 256
                                  // CUs; 256 / 384 / 768 / 1024 all measured slower (profiles/conv3x3_wgrad.md)
constexpr int WG_OOB = 0x7ffffff0;

__host__ __device__ constexpr int wg_xp(int S) { return S == 1 ? 192 : 160; }  // bytes per staged x pixel row

// Chunking of one shape (host and device agree through these numbers).  A
// chunk is a range of output columns [ct owt, ct owt + owt) of either part of
// one image's output rows (cpi row chunks per image, uc rows each) or -- only
// when it takes the full width -- of uc / OH whole images (cpi = 0).
struct WgPlan {
  int uc;      // output rows (units) per chunk
  int cpi;     // row chunks per image, 0: whole images per chunk
  int ct;      // column tiles per output row
  int owt;     // output columns per column tile
  int xpix;    // strip pixels a chunk stages at most
  int npad;    // dy pixels allocated (uc * owt rounded up to 16)
  int nch;     // chunks
  int cps;     // chunks per split
  int splits;  // workgroups along the reduction
  int lds;     // bytes
};

inline bool wg_plan(int N, int H, int W, int C, int K, int S, WgPlan* p) {
  const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;
  const int J = (H + 2) - (OH - 1) * S;  // strip rows from an image's last window origin to the next image's first (>= 3)
  int owt = OW, wps = 0;
  // strip rows of uc units: 3 for the first window, S per further unit of
  // the same image, J where the next unit starts a new image
  auto rows_of = [&](int uc, int images) { return 3 + (uc - 1) * S + (images - 1) * (J - S); };
  auto npad_of = [&](int uc) { return (uc * owt + 15) & ~15; };
  auto bytes = [&](int uc, int images) {
    return (long long)rows_of(uc, images) * wps * wg_xp(S) + (long long)npad_of(uc) * (WG_DP + 4);
  };
  auto fits = [&](int uc, int images) {
    return (long long)rows_of(uc, images) * wps <= 32 * WG_XL && npad_of(uc) <= 32 * WG_DL &&
           bytes(uc, images) <= WG_LDS;
  };
  for (int ct = 1;; ++ct) {  // the widest column tile one output row of which fits (owt = 1 always does)
    owt = (OW + ct - 1) / ct;
    wps = (owt - 1) * S + 3;
    if (fits(1, 1)) break;
  }
  p->owt = owt;
  p->ct = (OW + owt - 1) / owt;
  int uc = 1, images = 1;
  while (uc < OH && fits(uc + 1, 1)) ++uc;
  long long nch;
  if (uc == OH && p->ct == 1) {
    while (images < N && fits((images + 1) * OH, images + 1)) ++images;
    uc = images * OH;
    p->cpi = 0;
    nch = (N + images - 1) / images;
  } else {
    p->cpi = (OH + uc - 1) / uc;
    uc = (OH + p->cpi - 1) / p->cpi;  // even out the row chunks of an image
    nch = (long long)N * p->cpi * p->ct;
  }
  if (nch > 0x7fffffffLL) return false;
  p->uc = uc;
  p->xpix = rows_of(uc, images) * wps;
  p->npad = npad_of(uc);
  p->lds = (int)bytes(uc, images);
  const int tiles = (K / 64) * (C / 64);
  long long sp = (WG_TARGET + tiles - 1) / tiles;
  if (sp > nch) sp = nch;
  const long long cps = (nch + sp - 1) / sp;
  p->nch = (int)nch;
  p->cps = (int)cps;
  p->splits = (int)((nch + cps - 1) / cps);  // every split has at least one chunk
  return true;
}

inline bool wg_shape_ok(int N, int H, int W, int C, int K, int S) {
  if (N < 1 || H < 1 || W < 1 || C < 64 || C % 64 || K < 64 || K % 64 || (S != 1 && S != 2)) return false;
  const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;
  // 32-bit byte offsets, and the out-of-range offset must lie past both tensors
  if ((long long)N * H * W * C * 2 > WG_OOB || (long long)N * OH * OW * K * 2 > WG_OOB) return false;
  return true;
}

// One 32-row operand fragment with the MFMA k dimension along LDS rows:
// lane l holds channel (l & 31), pixels 8 (l >> 5) + 0..7.  a0 / a1: this
// lane's addresses in the blocks of pixels +0..3 / +4..7.
__device__ __forceinline__ wg_bf16x8 wg_tr(const unsigned char* a0, const unsigned char* a1) {
  const wg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)a0);
  const wg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)a1);
  const wg_u32x2 ul = __builtin_bit_cast(wg_u32x2, lo), uh = __builtin_bit_cast(wg_u32x2, hi);
  const wg_u32x4 o = {ul[0], ul[1], uh[0], uh[1]};
  return __builtin_bit_cast(wg_bf16x8, o);
}

// one chunk's place in the tensors (wave-uniform)
struct WgGeo {
  int u0, nu;     // first unit, units
  int ow0, owc;   // first output column, columns
  int vr0, rows;  // first strip row as a virtual row (image n row ih: n (H + 2) + ih + 1), strip rows
};

template <int S>
__global__ __launch_bounds__(WG_T) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_conv3x3_wgrad(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, float* __restrict__ ws, int N, int H, int W,
    int C, int OH, int OW, int K, int UC, int CPI, int CT, int OWT, int XPIX, int NPAD, int NCH, int CPS) {
  constexpr int XP = wg_xp(S);
  extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
  const int HP = H + 2, WPS = (OWT - 1) * S + 3;  // strip row pitch in pixels
  unsigned char* const Xs = wg_smem;                  // [XPIX][XP]
  unsigned char* const Ds = Xs + XPIX * XP;           // [NPAD][WG_DP]
  int* const Tab = reinterpret_cast<int*>(Ds + NPAD * WG_DP);  // [NPAD]

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int mi = wv >> 1, ni = wv & 1;
  const int tiles_c = C / 64, tiles = (K / 64) * tiles_c;
  const int sp = blockIdx.x / tiles, tile = blockIdx.x - sp * tiles;
  const int k0 = (tile / tiles_c) * 64, c0 = (tile % tiles_c) * 64;
  const int NU = N * OH;

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), 0, N * H * W * C * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t dr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(dy), 0, N * OH * OW * K * 2, 0x00020000);

  wg_f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = wg_f32x16{};

  // transposed-read geometry: 16-lane group g takes pixels 8 (g >> 1) + 4 j +
  // q, channels 16 (g & 1) + 4 p .. + 3 of the wave's 32; lane 4 q + p of the
  // group supplies the address of pixel row q
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int pix_l = 8 * (g >> 1) + q;
  const int col_l = (16 * (g & 1) + 4 * pp) * 2;
  const unsigned char* const a_base = Ds + pix_l * WG_DP + mi * 64 + col_l;
  const unsigned char* const b_base = Xs + ni * 64 + col_l;

  const int ch = tid & 7, prow = tid >> 3;  // staging: 16-byte chunk, pixel within a pass of 32
  const int q32 = 32 / WPS, r32 = 32 - q32 * WPS;  // a pass of 32 strip pixels in rows and columns
  const int prow_r = prow / WPS, prow_c = prow - prow_r * WPS;
  const int cbeg = sp * CPS, cend = min(cbeg + CPS, NCH);

  auto geo = [&](int cc) {
    WgGeo o;
    const int rc = cc / CT, ct = cc - rc * CT;
    o.ow0 = ct * OWT;
    o.owc = min(OWT, OW - o.ow0);
    int u1;
    if (CPI) {  // rows [o0, o0 + UC) of image rc / CPI
      const int n = rc / CPI, o0 = (rc - n * CPI) * UC;
      o.u0 = n * OH + o0;
      u1 = n * OH + min(o0 + UC, OH);
    } else {  // whole images
      o.u0 = rc * UC;
      u1 = min(o.u0 + UC, NU);
    }
    o.nu = u1 - o.u0;
    const int n0 = o.u0 / OH, oh0 = o.u0 - n0 * OH;
    const int nl = (u1 - 1) / OH, ohl = (u1 - 1) - nl * OH;
    o.vr0 = n0 * HP + oh0 * S;
    o.rows = min(nl * HP + ohl * S + 3 - o.vr0, XPIX / WPS);  // the bound cannot bind (wg_plan); it keeps the LDS
    o.nu = min(o.nu, NPAD / o.owc);                           // writes in range regardless
    return o;
  };

  // The chunk's operands, global -> registers.  Every load is issued
  // whatever the chunk's size (rows past it, and all of them when !live, at
  // the out-of-range offset): a conditionally filled register array would be
  // demoted to scratch.
  wg_u32x4 rx[WG_XL], rd[WG_DL];
#define WG_LOAD(G, live)                                                                                  \
  {                                                                                                       \
    int row_ = prow_r, col_ = prow_c;                                                                     \
    int n_ = (G.vr0 + row_) / HP, vrow_ = G.vr0 + row_ - n_ * HP;                                         \
    const int iw0_ = G.ow0 * S - 1;                                                                       \
    _Pragma("unroll") for (int i = 0; i < WG_XL; ++i) {                                                   \
      const int ih_ = vrow_ - 1, iw_ = iw0_ + col_;                                                       \
      const bool ok_ = (live) && row_ < G.rows && (unsigned)ih_ < (unsigned)H && (unsigned)iw_ < (unsigned)W; \
      rx[i] = __builtin_bit_cast(wg_u32x4, __builtin_amdgcn_raw_buffer_load_b128(                         \
                                               xr, ok_ ? (((n_ * H + ih_) * W + iw_) * C + c0 + ch * 8) * 2 : WG_OOB, 0, 0)); \
      col_ += r32;                                                                                        \
      int d_ = q32;                                                                                       \
      if (col_ >= WPS) {                                                                                  \
        col_ -= WPS;                                                                                      \
        ++d_;                                                                                             \
      }                                                                                                   \
      row_ += d_;                                                                                         \
      vrow_ += d_;                                                                                        \
      while (vrow_ >= HP) {                                                                               \
        vrow_ -= HP;                                                                                      \
        ++n_;                                                                                             \
      }                                                                                                   \
    }                                                                                                     \
    const int npix_ = G.nu * G.owc;                                                                       \
    _Pragma("unroll") for (int i = 0; i < WG_DL; ++i) {                                                   \
      const int pix_ = i * 32 + prow, du_ = pix_ / G.owc, ow_ = pix_ - du_ * G.owc;                       \
      rd[i] = __builtin_bit_cast(                                                                         \
          wg_u32x4, __builtin_amdgcn_raw_buffer_load_b128(                                                \
                        dr, (live) && pix_ < npix_ ? (((G.u0 + du_) * OW + G.ow0 + ow_) * K + k0 + ch * 8) * 2 : WG_OOB, 0, 0)); \
    }                                                                                                     \
  }

  WgGeo gn = geo(cbeg);
  WG_LOAD(gn, true)
  for (int cc = cbeg; cc < cend; ++cc) {
    const WgGeo gc = gn;
    const int npix = gc.nu * gc.owc, np16 = (npix + 15) & ~15, sp_pix = gc.rows * WPS;
    if (cc != cbeg) __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < WG_XL; ++i) {
      const int pix = i * 32 + prow;
      if (pix < sp_pix) *reinterpret_cast<wg_u32x4*>(Xs + pix * XP + ch * 16) = rx[i];
    }
#pragma unroll
    for (int i = 0; i < WG_DL; ++i) {
      const int pix = i * 32 + prow;
      if (pix < np16) *reinterpret_cast<wg_u32x4*>(Ds + pix * WG_DP + ch * 16) = rd[i];  // zeros past npix
    }
    if (tid < np16) {  // np16 <= 32 WG_DL <= WG_T
      int off = 0;
      if (tid < npix) {
        const int du = tid / gc.owc, ow = tid - du * gc.owc;
        const int u = gc.u0 + du, n = u / OH, oh = u - n * OH;
        off = ((n * HP + oh * S - gc.vr0) * WPS + ow * S) * XP;
      }
      Tab[tid] = off;
    }
    __syncthreads();
    const bool more = cc + 1 < cend;
    gn = geo(more ? cc + 1 : cc);
    WG_LOAD(gn, more)  // in flight under this chunk's MFMAs

    // 16 pixels per step: one dy fragment, nine x fragments (one per tap)
    const int steps = np16 >> 4;
    for (int st = 0; st < steps; ++st) {
      const int t0 = Tab[st * 16 + pix_l], t1 = Tab[st * 16 + pix_l + 4];
      const unsigned char* const a0 = a_base + st * 16 * WG_DP;
      const wg_bf16x8 af = wg_tr(a0, a0 + 4 * WG_DP);
      wg_bf16x8 bf[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int toff = ((t / 3) * WPS + (t % 3)) * XP;
        bf[t] = wg_tr(b_base + t0 + toff, b_base + t1 + toff);
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[t], acc[t], 0, 0, 0);
    }
  }
#undef WG_LOAD

  // partial sums: ws[sp][k][tap][c]; a lane's 32 columns are contiguous c
  float* const out = ws + (size_t)sp * K * 9 * C;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = k0 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
      out[((size_t)k * 9 + t) * C + c0 + ni * 32 + fr] = acc[t][e];
    }
}

// dw[i] = ws[0][i] + ws[1][i] + ... in split order (n % 4 == 0)
__global__ __launch_bounds__(256) void k_conv3x3_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw,
                                                              int n, int splits) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float4 s = *reinterpret_cast<const float4*>(ws + i);
  for (int j = 1; j < splits; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(ws + (size_t)j * n + i);
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  *reinterpret_cast<float4*>(dw + i) = s;
}

template <int S>
int wg_launch(const void* x, const void* dy, float* dw, float* ws, int N, int H, int W, int C, int K, const WgPlan& p,
              hipStream_t s) {
  const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;
  const int tiles = (K / 64) * (C / 64);
  const long long blocks = (long long)tiles * p.splits;
  if (blocks > 0x7fffffffLL) return -1;
  static bool attr = false;
  if (!attr) {  // more than 64 KB of dynamic LDS
    (void)hipFuncSetAttribute((const void*)k_conv3x3_wgrad<S>, hipFuncAttributeMaxDynamicSharedMemorySize, 81920);
    attr = true;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_conv3x3_wgrad<S>), dim3((unsigned)blocks), dim3(WG_T), (size_t)p.lds, s,
                     reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(dy), ws, N, H, W, C, OH,
                     OW, K, p.uc, p.cpi, p.ct, p.owt, p.xpix, p.npad, p.nch, p.cps);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const int n = K * 9 * C;
  hipLaunchKernelGGL(k_conv3x3_wgrad_reduce, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, ws, dw, n,
                     p.splits);
  return (int)hipGetLastError();
}

}  // namespace

#define PTO_API extern "C" __attribute__((visibility("default")))

// Workgroups along the pixel reduction for this shape (a function of the
// shape and of compile-time constants only), i.e. the fp32 workspace holds
// splits * K * 9 * C floats; -1 for a shape the kernel does not take.
PTO_API int pto_conv3x3_wgrad_splits(int N, int H, int W, int C, int K, int stride) {
  WgPlan p;
  if (!wg_shape_ok(N, H, W, C, K, stride) || !wg_plan(N, H, W, C, K, stride, &p)) return -1;
  return p.splits;
}

// dw[K][3][3][C] (fp32) = weight gradient of conv3x3(x[N][H][W][C], .) for
// dy[N][OH][OW][K], pad 1, stride 1 or 2, bf16 channels-last operands; ws:
// pto_conv3x3_wgrad_splits(...) * K * 9 * C floats of scratch (any content).
PTO_API int pto_conv3x3_wgrad(const void* x, const void* dy, float* dw, float* ws, int N, int H, int W, int C, int K,
                              int stride, hipStream_t s) {
  WgPlan p;
  if (!x || !dy || !dw || !ws || !wg_shape_ok(N, H, W, C, K, stride) || !wg_plan(N, H, W, C, K, stride, &p)) return -1;
  if ((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)dw) | ((uintptr_t)ws)) & 15) return -1;
  return stride == 1 ? wg_launch<1>(x, dy, dw, ws, N, H, W, C, K, p, s)
                     : wg_launch<2>(x, dy, dw, ws, N, H, W, C, K, p, s);
}
