// bf16 GEMM with fp32 accumulation (v_mfma_f32_32x32x16_bf16) for the three
// products of a bias-free linear layer, each from the layouts the model
// stores -- no transposed copy of a weight or an activation is needed:
//
//   form 0, NT: C[M,N] = A[M,K] . B[N,K]^T   forward x W^T (dgrad from a W^T copy)
//   form 1, NN: C[M,K] = A[M,N] . B[N,K]     dgrad dY W
//   form 2, TN: C[N,K] = A[M,N]^T . B[M,K]   wgrad dY^T X
//
// One kernel template computes out[R][CN] = sum_k a(r, k) b(k, c) over a
// contraction of KC; each operand's loader is one of two kinds:
//
//   k-major   the operand is contiguous along the contraction index
//             (element (r, k) at p[r ld + k]).  Staged as [rows][64 k];
//             lane l reads its fragment (row l & 31, k = 8 (l >> 5) + 0..7:
//             16 contiguous bytes) with one ds_read_b128.
//   mn-major  the operand is contiguous along the output index (element
//             (r, k) at p[k ld + r]).  Staged as stored, [64 k][rows],
//             and the same fragment comes from two ds_read_b64_tr_b16, each
//             delivering 4 k-rows x 16 columns column-major to a 16-lane
//             group (lane 4 q + p of a group supplies the address of k-row
//             q, columns 4 p .. 4 p + 3).  Every lane is active at these
//             reads: the k-loop is workgroup-uniform and edge tiles are
//             handled by clamped loads, not by masks.
//
// NT = (k-major, k-major), NN = (k-major, mn-major), TN = (mn-major, mn-major).
//
// Two tiles, chosen from the form and the shape alone (gm_big_tile):
//   128 x 128  256 threads = 4 waves as 2 x 2, wave (wm, wn) owns 64 x 64 as
//              2 x 2 MFMA tiles of 32 x 32 (64 accumulator registers); per
//              k-step 4 fragment reads feed 4 MFMAs.  72 - 80 KB of LDS, two
//              workgroups per CU.  Takes every shape; small outputs still
//              fill the machine.
//   256 x 256  512 threads = 8 waves as 2 x 4, a wave owns 128 x 64 as 4 x 2
//              MFMA tiles (128 accumulator registers); 6 fragment reads feed
//              8 MFMAs and each staged byte is used twice as often.  144 KB of
//              LDS, one workgroup per CU.  Used by NN and TN once the output
//              has 256 such tiles (one per CU).
// BK = 64 in both: a k-tile is 4 k-steps of the 32x32x16 MFMA.
//
// Pipeline: two LDS buffers and one register set.  While tile t multiplies
// out of buffer t & 1, tile t + 1 is in flight global -> registers (8 loads of
// 16 bytes per thread); it is written to buffer (t + 1) & 1 after the MFMAs
// and one barrier ends the step.  That buffer was last read in step t - 1,
// before the previous barrier.
//
// Edges: the contraction is a multiple of 64, so no k-tile is partial.  An
// output row or column past the end only ever feeds output elements past the
// end, so edge tiles load from a clamped (valid) row / column instead of
// zero-filling, and the epilogue stores under a mask.
//
// LDS pitches and bank conflicts (bank = (addr / 4) % 64):
//   k-major rows are 144 bytes apart (128 of data).  A ds_read_b128 is served
//   per 16-lane group; its lanes read 16 consecutive rows at one k offset,
//   i.e. the 16-byte slots 9 r mod 16 of the 256-byte bank row -- 9 is odd,
//   so all 16 differ: conflict-free.
//   mn-major rows are 2 rows + 64 bytes apart (320 for 256 of data, 576 for
//   512: both 64 mod 256).  A transposed read is
//   counted per 32-lane half, which takes 4 consecutive k-rows x 64 contiguous
//   bytes; the rows start at 0, 64, 128, 192 (mod 256), four disjoint 64-byte
//   bank ranges: conflict-free at any column offset that is a multiple of 64
//   bytes (the wave's are).
//   Staging writes (ds_write_b128, 16 lanes = 2 rows x 128 bytes or 1 row x
//   256 bytes) are conflict-free on the mn-major image and 2-way on one slot
//   of the k-major image.
//
// Workgroup order: the launch index is first remapped so that the workgroups
// one XCD receives (index mod 8) form one contiguous range of tile numbers
// (the bijective form: the tile count need not be a multiple of 8), then tile
// numbers walk groups of 8 tile rows column by column, so the tiles an XCD's
// L2 serves at a time share A and B panels.
//
// No split-K and no atomics: every output element is summed by one wave in
// one fixed order, so results are bitwise repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __bf16 gm_bf16x8 __attribute__((ext_vector_type(8)));
typedef float gm_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned gm_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned gm_u32x2 __attribute__((ext_vector_type(2)));
typedef short gm_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gm_s16x4 gm_lds_s16x4;

constexpr int GM_BK = 64;      // contraction elements per step
constexpr int GM_PK = 144;     // bytes per staged row, k-major image [rows][64]
constexpr int GM_GROUP = 8;    // tile rows walked together
constexpr int GM_NL = 4;       // 16-byte loads per thread per operand per k-tile (64 threads per 32 rows)
constexpr int GM_BIG_MIN = 256;  // 256 x 256 tiles from this many of them: one per CU

// bytes per staged k-row of an mn-major image [64][rows]: 64 mod 256, see above
__host__ __device__ constexpr int gm_pm(int rows) { return rows * 2 + 64; }
__host__ __device__ constexpr int gm_img(bool mn, int rows) { return mn ? GM_BK * gm_pm(rows) : rows * GM_PK; }

// One 32-row fragment of an mn-major image: a0 / a1 are this lane's addresses
// in the blocks of k-rows +0..3 / +4..7.
__device__ __forceinline__ gm_bf16x8 gm_tr(const unsigned char* a0, const unsigned char* a1) {
  const gm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gm_lds_s16x4*)a0);
  const gm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gm_lds_s16x4*)a1);
  const gm_u32x2 ul = __builtin_bit_cast(gm_u32x2, lo), uh = __builtin_bit_cast(gm_u32x2, hi);
  const gm_u32x4 o = {ul[0], ul[1], uh[0], uh[1]};
  return __builtin_bit_cast(gm_bf16x8, o);
}

// Loader of one operand's ROWS x 64 (k) tile by T = 2 ROWS threads.  ext: the
// operand's extent along the output index, row0: the tile's first row.
template <bool MN, int ROWS>
struct GmOperand {
  static constexpr int GM_T = 2 * ROWS, GM_PM = gm_pm(ROWS), PIECES = ROWS / 8;
  const uint16_t* src[GM_NL];  // this thread's 16-byte pieces of the current k-tile
  int dst[GM_NL];              // their byte offsets in the LDS image
  size_t step;                 // elements from one k-tile to the next
  int frag;                    // this lane's fragment offset in the image, k-step 0, row block 0

  __device__ __forceinline__ void init(const uint16_t* p, long long ld, int ext, int row0, int wrow, int tid,
                                       int lane) {
#pragma unroll
    for (int i = 0; i < GM_NL; ++i) {
      const int c = i * GM_T + tid;
      if (MN) {  // [64 k][ROWS]: ROWS / 8 pieces per k-row
        const int kr = c / PIECES, ch = c % PIECES;
        const int col = min(row0 + ch * 8, ext - 8);  // ext is a multiple of 8
        src[i] = p + (size_t)kr * ld + col;
        dst[i] = kr * GM_PM + ch * 16;
      } else {  // [ROWS][64 k]: 8 pieces per row
        const int r = c >> 3, ch = c & 7;
        const int row = min(row0 + r, ext - 1);
        src[i] = p + (size_t)row * ld + ch * 8;
        dst[i] = r * GM_PK + ch * 16;
      }
    }
    step = MN ? (size_t)GM_BK * ld : (size_t)GM_BK;
    if (MN) {
      const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
      frag = (8 * (g >> 1) + q) * GM_PM + (wrow + 16 * (g & 1) + 4 * pp) * 2;
    } else {
      frag = (wrow + (lane & 31)) * GM_PK + (lane >> 5) * 16;
    }
  }

  __device__ __forceinline__ void load(gm_u32x4 (&r)[GM_NL]) {
#pragma unroll
    for (int i = 0; i < GM_NL; ++i) {
      r[i] = *reinterpret_cast<const gm_u32x4*>(src[i]);
      src[i] += step;
    }
  }

  __device__ __forceinline__ void store(unsigned char* img, const gm_u32x4 (&r)[GM_NL]) const {
#pragma unroll
    for (int i = 0; i < GM_NL; ++i) *reinterpret_cast<gm_u32x4*>(img + dst[i]) = r[i];
  }

  // fragment of row block rb (32 rows) at k-step ks (16 k)
  __device__ __forceinline__ gm_bf16x8 fragment(const unsigned char* img, int rb, int ks) const {
    if (MN) {
      const unsigned char* a0 = img + frag + ks * 16 * GM_PM + rb * 64;
      return gm_tr(a0, a0 + 4 * GM_PM);
    }
    return *reinterpret_cast<const gm_bf16x8*>(img + frag + rb * 32 * GM_PK + ks * 32);
  }
};

__device__ __forceinline__ void gm_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void gm_store(uint16_t* p, float v) {
  *p = __builtin_bit_cast(uint16_t, (__bf16)v);  // round to nearest even
}

// BM x BN output tile on WM x WN waves; BM = BN (both loaders are fed by all
// 2 BM threads), wave tile (BM / WM) x (BN / WN) as MI x NI MFMA tiles
template <bool A_MN, bool B_MN, typename OutT, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void k_gemm_bf16(const uint16_t* __restrict__ A, long long lda,
                                                    const uint16_t* __restrict__ B, long long ldb,
                                                    OutT* __restrict__ C, long long ldc, int R, int CN, int KC,
                                                    int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_smem[];
  constexpr int IMG_A = gm_img(A_MN, BM), IMG_B = gm_img(B_MN, BN), BUF = IMG_A + IMG_B;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  static_assert(BM == BN && 64 * WM * WN == 2 * BM, "both loaders use every thread");

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv / WN, wn = wv % WN;

  // XCD remap (bijective), then grouped tile order
  const int nwg = tiles_m * tiles_n;
  const int orig = blockIdx.x, xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
  const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
  const int per_group = GM_GROUP * tiles_n;
  const int gid = wg / per_group, in_g = wg - gid * per_group;
  const int gsz = min(tiles_m - gid * GM_GROUP, GM_GROUP);
  const int tm = gid * GM_GROUP + in_g % gsz, tn = in_g / gsz;
  const int row0 = tm * BM, col0 = tn * BN;

  GmOperand<A_MN, BM> la;
  GmOperand<B_MN, BN> lb;
  la.init(A, lda, R, row0, wm * TM, tid, lane);
  lb.init(B, ldb, CN, col0, wn * TN, tid, lane);

  gm_f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = gm_f32x16{};

  gm_u32x4 ra[GM_NL], rb[GM_NL];
  const int nt = KC / GM_BK;

  auto multiply = [&](const unsigned char* buf) {
    const unsigned char* const ia = buf;
    const unsigned char* const ib = buf + IMG_A;
#pragma unroll
    for (int ks = 0; ks < GM_BK / 16; ++ks) {
      gm_bf16x8 af[MI], bf[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = la.fragment(ia, i, ks);
#pragma unroll
      for (int j = 0; j < NI; ++j) bf[j] = lb.fragment(ib, j, ks);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  la.load(ra);
  lb.load(rb);
  la.store(gm_smem, ra);
  lb.store(gm_smem + IMG_A, rb);
  __syncthreads();
  for (int t = 0; t + 1 < nt; ++t) {
    la.load(ra);  // tile t + 1, in flight under tile t's MFMAs
    lb.load(rb);
    multiply(gm_smem + (t & 1) * BUF);
    unsigned char* const nxt = gm_smem + ((t + 1) & 1) * BUF;
    la.store(nxt, ra);
    lb.store(nxt + IMG_A, rb);
    __syncthreads();
  }
  multiply(gm_smem + ((nt - 1) & 1) * BUF);

  // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = col0 + wn * TN + j * 32 + fr;
    if (col >= CN) continue;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = row0 + wm * TM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (row < R) gm_store(C + (size_t)row * ldc + col, acc[i][j][e]);
      }
  }
}

struct GmShape {
  int R, CN, KC;     // output rows, output columns, contraction
  bool a_mn, b_mn;
  long long wa, wb;  // inner (contiguous) extent of A and B as stored
};

inline bool gm_shape(int form, long long M, long long N, long long K, long long lda, long long ldb, long long ldc,
                     GmShape* s) {
  if (form < 0 || form > 2 || M < 1 || N < 1 || K < 1 || M > 0x7fffffffLL || N > 0x7fffffffLL || K > 0x7fffffffLL)
    return false;
  long long R, CN, KC;
  if (form == 0) {  // C[M,N] = A[M,K] B[N,K]^T
    R = M, CN = N, KC = K;
    s->a_mn = false, s->b_mn = false, s->wa = K, s->wb = K;
  } else if (form == 1) {  // C[M,K] = A[M,N] B[N,K]
    R = M, CN = K, KC = N;
    s->a_mn = false, s->b_mn = true, s->wa = N, s->wb = K;
  } else {  // C[N,K] = A[M,N]^T B[M,K]
    R = N, CN = K, KC = M;
    s->a_mn = true, s->b_mn = true, s->wa = N, s->wb = K;
  }
  if (CN % 64 || KC % GM_BK) return false;
  if (s->a_mn && R % 8) return false;  // 16-byte pieces along the output rows
  if (lda % 8 || ldb % 8 || ldc % 8 || lda < s->wa || ldb < s->wb || ldc < CN) return false;
  const long long tiles = ((R + 127) / 128) * ((CN + 127) / 128);
  if (tiles > 0x7fffffffLL) return false;
  s->R = (int)R, s->CN = (int)CN, s->KC = (int)KC;
  return true;
}

template <bool A_MN, bool B_MN, typename OutT, int BM, int BN, int WM, int WN>
int gm_launch_tile(const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc,
                   const GmShape& s, hipStream_t st) {
  constexpr int LDS = 2 * (gm_img(A_MN, BM) + gm_img(B_MN, BN));  // above the 64 KB a kernel gets by default
  static const int attr = (int)hipFuncSetAttribute((const void*)k_gemm_bf16<A_MN, B_MN, OutT, BM, BN, WM, WN>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  if (attr) return attr;
  const int tiles_m = (s.R + BM - 1) / BM, tiles_n = (s.CN + BN - 1) / BN;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gemm_bf16<A_MN, B_MN, OutT, BM, BN, WM, WN>),
                     dim3((unsigned)(tiles_m * tiles_n)), dim3(64 * WM * WN), (size_t)LDS, st,
                     reinterpret_cast<const uint16_t*>(A), lda, reinterpret_cast<const uint16_t*>(B), ldb,
                     reinterpret_cast<OutT*>(C), ldc, s.R, s.CN, s.KC, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

// The tile is a function of the form and the shape alone: 256 x 256 (8 waves
// as 2 x 4, a wave 128 x 64) once there is one such tile per CU, else
// 128 x 128.  Measured on the Llama-3-8B shapes (profiles/gemm_bf16.md): the
// large tile gains 10 - 25 % where an operand is mn-major (NN, TN) and loses
// 30 - 45 % where both are k-major (NT), which therefore keeps the small one.
inline bool gm_big_tile(const GmShape& s) {
  return (s.a_mn || s.b_mn) && (long long)((s.R + 255) / 256) * ((s.CN + 255) / 256) >= GM_BIG_MIN;
}

template <bool A_MN, bool B_MN, typename OutT>
int gm_launch(const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc, const GmShape& s,
              hipStream_t st) {
  if constexpr (A_MN || B_MN) {
    if (gm_big_tile(s)) return gm_launch_tile<A_MN, B_MN, OutT, 256, 256, 2, 4>(A, lda, B, ldb, C, ldc, s, st);
  }
  return gm_launch_tile<A_MN, B_MN, OutT, 128, 128, 2, 2>(A, lda, B, ldb, C, ldc, s, st);
}

template <typename OutT>
int gm_dispatch(int form, const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc,
                const GmShape& s, hipStream_t st) {
  if (form == 0) return gm_launch<false, false, OutT>(A, lda, B, ldb, C, ldc, s, st);
  if (form == 1) return gm_launch<false, true, OutT>(A, lda, B, ldb, C, ldc, s, st);
  return gm_launch<true, true, OutT>(A, lda, B, ldb, C, ldc, s, st);
}

}  // namespace

#define PTO_API extern "C" __attribute__((visibility("default")))

// 1 if pto_gemm_bf16 takes this form / shape / row strides (in elements), else
// 0.  M, N, K name the dimensions as in the table at the top of this file;
// the contraction (K, N, M for forms 0, 1, 2) and the output columns must be
// multiples of 64, the output rows are free (a multiple of 8 for form 2), and
// every row stride is a multiple of 8 and at least the row's width.
PTO_API int pto_gemm_bf16_supported(int form, long long M, long long N, long long K, long long lda, long long ldb,
                                    long long ldc) {
  GmShape s;
  return gm_shape(form, M, N, K, lda, ldb, ldc, &s) ? 1 : 0;
}

// C = the product of form `form` (0 NT, 1 NN, 2 TN) of bf16 A and B, summed in
// fp32, written as bf16 or (out_is_f32) fp32.  Unit inner strides, row strides
// in elements, 16-byte aligned base pointers.  -1, with nothing launched, for
// anything pto_gemm_bf16_supported refuses or a misaligned / null pointer.
PTO_API int pto_gemm_bf16(int form, const void* A, long long lda, const void* B, long long ldb, void* C,
                          long long ldc, int out_is_f32, long long M, long long N, long long K, hipStream_t stream) {
  GmShape s;
  if (!A || !B || !C || !gm_shape(form, M, N, K, lda, ldb, ldc, &s)) return -1;
  if ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C)) & 15) return -1;
  return out_is_f32 ? gm_dispatch<float>(form, A, lda, B, ldb, C, ldc, s, stream)
                    : gm_dispatch<uint16_t>(form, A, lda, B, ldb, C, ldc, s, stream);
}
