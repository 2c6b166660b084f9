// FP8 linear layers: per-tensor power-of-two quantisers (e4m3 / e5m2) and a
// K = 128 MFMA GEMM on 8-bit operands (v_mfma_scale_f32_16x16x128_f8f6f4).
//
// Numerics (ops/fp8.py states them once): scale 2^e, e the largest integer with
// amax 2^e <= FMAX (448 for e4m3, 57344 for e5m2), clamped to [-64, 64], 0 for
// amax == 0, derived from the exponent and mantissa bits of amax; q = rne(x 2^e)
// by v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32; the GEMM accumulates in fp32 and its
// epilogue multiplies by 2^-(ea + eb), adds the fp32 bias and rounds once to bf16.
//
// Quantising is two plain launches: fp8_amax_kernel leaves one partial per
// workgroup (at most kFp8MaxParts), every workgroup of the quantiser reduces the
// partials itself in its prologue (a max of |x| bit patterns: any order gives
// the same value) and workgroup 0 writes 2^-e to the one-element scale tensor.
// Nothing is read by the host.
//
// gemm_nt_fp8_kernel: 256 threads, a 128 x 128 output tile, one 128-byte K slice
// per step (one MFMA deep), every wave a 64 x 64 quadrant (4 x 4 accumulator
// tiles, 64 registers).  Both operand tiles come by LDS-DMA into two 32 KiB
// stages; the next slice is issued right after the barrier, before the current
// slice's MFMAs.  Rows lie 128 bytes apart in LDS with their 16-byte chunks
// XOR-ed by (row >> 1) & 7, and lane (fr, fq) reads chunks fq and 4 + fq of its
// row -- the read pattern gemm_nt.h measured conflict-free -- instead of the 32
// contiguous bytes 32 fq .. 32 fq + 31.  That is a permutation of the K index
// applied to both operands alike: the instruction multiplies byte b of lane
// group fq of one operand with byte b of lane group fq of the other, so the sum
// over the slice is the same.  The MFMA is issued swapped (weight rows as its
// first operand), so a lane ends with 4 consecutive output columns of one row.
// Tail rows of A are clamped to row M - 1 on load (in bounds; rows are
// independent) and skipped on store.
#include <hip/hip_runtime.h>

#include "gemm_common.h"

namespace gk {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------
// amax + quantise
// ---------------------------------------------------------------------------
// max |x| bit pattern of 16 consecutive elements (n % 16 == 0, 16-byte loads)
template <bool BF16>
__device__ __forceinline__ void load16(const void* x, int64_t v, float* f) {
  if constexpr (BF16) {
    const u32x4* p = reinterpret_cast<const u32x4*>(x) + 2 * v;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 w = p[h];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[8 * h + 2 * i] = __uint_as_float(w[i] << 16);
        f[8 * h + 2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
      }
    }
  } else {
    const f32x4* p = reinterpret_cast<const f32x4*>(x) + 4 * v;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const f32x4 w = p[h];
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * h + i] = w[i];
    }
  }
}

__device__ __forceinline__ uint32_t block_max_u32(uint32_t k, uint32_t* sh) {
  k = wave_max(k);
  __syncthreads();
  if (lane_id() == 0) sh[wave_id()] = k;
  __syncthreads();
  uint32_t r = sh[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) r = sh[w] > r ? sh[w] : r;
  return r;
}

template <bool BF16>
__global__ void __launch_bounds__(kBlock) fp8_amax_kernel(const void* __restrict__ x, int64_t nvec,
                                                          uint32_t* __restrict__ partials) {
  __shared__ uint32_t sh[kWavesPerBlock];
  uint32_t k = 0u;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kBlock) {
    float f[16];
    load16<BF16>(x, v, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t a = abs_key(f[i]);
      k = a > k ? a : k;
    }
  }
  k = block_max_u32(k, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = k;
}

// the scale exponent from the bits of amax = m 2^x, 1 <= m < 2: FMAX = 1.75 2^P,
// so e = P - x when m <= 1.75 and P - x - 1 otherwise (zero: 0; subnormal amax
// and everything else out of range: the clamp)
template <int FMT>
__device__ __forceinline__ int fp8_exp(uint32_t amax_bits) {
  constexpr int P = FMT == kFp8E4M3 ? 8 : 15;
  if (amax_bits == 0u) return 0;
  const int x = (int)(amax_bits >> 23) - 127;
  int e = P - x - ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < -64 ? -64 : e;
  return e > 64 ? 64 : e;
}

// every workgroup: partials -> amax -> e; returns 2^e, workgroup 0 writes 2^-e
template <int FMT>
__device__ __forceinline__ float fp8_scale_prologue(const uint32_t* __restrict__ partials, int nparts,
                                                    float* __restrict__ scale, bool writer, uint32_t* sh) {
  uint32_t k = 0u;
  for (int i = threadIdx.x; i < nparts; i += kBlock) k = partials[i] > k ? partials[i] : k;
  k = block_max_u32(k, sh);
  const int e = fp8_exp<FMT>(k);
  if (writer && threadIdx.x == 0) *scale = __uint_as_float((uint32_t)(127 - e) << 23);
  return __uint_as_float((uint32_t)(127 + e) << 23);
}

// 16 scaled values -> 16 bytes, four per v_cvt_pk pair
template <int FMT>
__device__ __forceinline__ u32x4 cvt16(const float* f, float mul) {
  u32x4 q;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int w = 0;
    if constexpr (FMT == kFp8E4M3) {
      w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i] * mul, f[4 * i + 1] * mul, w, false);
      w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2] * mul, f[4 * i + 3] * mul, w, true);
    } else {
      w = __builtin_amdgcn_cvt_pk_bf8_f32(f[4 * i] * mul, f[4 * i + 1] * mul, w, false);
      w = __builtin_amdgcn_cvt_pk_bf8_f32(f[4 * i + 2] * mul, f[4 * i + 3] * mul, w, true);
    }
    q[i] = (uint32_t)w;
  }
  return q;
}

template <int FMT, bool BF16>
__global__ void __launch_bounds__(kBlock) fp8_quant_kernel(const void* __restrict__ x, int64_t nvec,
                                                           const uint32_t* __restrict__ partials, int nparts,
                                                           u32x4* __restrict__ q, float* __restrict__ scale) {
  __shared__ uint32_t sh[kWavesPerBlock];
  const float mul = fp8_scale_prologue<FMT>(partials, nparts, scale, blockIdx.x == 0, sh);
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kBlock) {
    float f[16];
    load16<BF16>(x, v, f);
    q[v] = cvt16<FMT>(f, mul);
  }
}

// The weight [N, K] (K % 16 == 0, any N): one 64 x 64 tile per workgroup, read
// once, written as W8 [N, K] and -- through an LDS tile read column-wise -- as
// W8T [K, N] with the same scale.  Rows of W8T are 16-byte aligned only when
// N % 16 == 0; otherwise the transposed bytes are stored one by one.
constexpr int kQtTile = 64;
constexpr int kQtPitch = 80;   // 16-byte aligned rows, column reads 20 banks apart

template <bool BF16>
__global__ void __launch_bounds__(kBlock) fp8_quant_t_kernel(const void* __restrict__ w, int N, int K,
                                                             const uint32_t* __restrict__ partials, int nparts,
                                                             uint8_t* __restrict__ w8, uint8_t* __restrict__ w8t,
                                                             float* __restrict__ scale) {
  __shared__ uint32_t sh[kWavesPerBlock];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kQtTile * kQtPitch];
  const float mul =
      fp8_scale_prologue<kFp8E4M3>(partials, nparts, scale, blockIdx.x == 0 && blockIdx.y == 0, sh);
  const int r = threadIdx.x >> 2, cs = (threadIdx.x & 3) * 16;
  const int n0 = blockIdx.y * kQtTile, k0 = blockIdx.x * kQtTile;
  u32x4 q = u32x4{0u, 0u, 0u, 0u};
  if (n0 + r < N && k0 + cs < K) {
    const int64_t at = (int64_t)(n0 + r) * K + k0 + cs;   // a multiple of 16
    float f[16];
    load16<BF16>(w, at >> 4, f);
    q = cvt16<kFp8E4M3>(f, mul);
    *reinterpret_cast<u32x4*>(w8 + at) = q;
  }
  *reinterpret_cast<u32x4*>(tile + r * kQtPitch + cs) = q;
  __syncthreads();
  // thread (r, cs) now owns row k0 + r of W8T, columns n0 + cs .. + 15
  if (k0 + r >= K) return;
  uint8_t b[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = tile[(cs + j) * kQtPitch + r];
  uint8_t* dst = w8t + (int64_t)(k0 + r) * N + n0 + cs;
  if ((N & 15) == 0) {
    if (n0 + cs < N) {
      u32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
      *reinterpret_cast<u32x4*>(dst) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (n0 + cs + j < N) dst[j] = b[j];
  }
}

int fp8_grid(int64_t nvec) {
  const int64_t g = (nvec + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > kFp8MaxParts ? kFp8MaxParts : g));
}

// ---------------------------------------------------------------------------
// gemm_nt_fp8: C[M, N] = A[M, K] B[N, K]^T on 8-bit operands
// ---------------------------------------------------------------------------
struct Fp8Cfg {
  static constexpr int THREADS = 256, NW = 4;
  static constexpr int BM = 128, BN = 128, KS = 128;   // KS: bytes (= elements) of one K slice row
  static constexpr int ASTAGE = BM * KS, BSTAGE = BN * KS, STAGE = ASTAGE + BSTAGE;
  static constexpr int LDS = 2 * STAGE;                // 64 KiB: two workgroups per CU
  static constexpr int LPW = STAGE / 1024 / NW;        // 1-KiB LDS-DMA instructions per wave per stage
  static constexpr int LPWA = ASTAGE / 1024 / NW;      // of which A rows
};

__device__ __forceinline__ int fp8_swz(int r) { return (r >> 1) & 7; }

template <int AFMT>
__global__ void __launch_bounds__(Fp8Cfg::THREADS) gemm_nt_fp8_kernel(Fp8GemmArgs g) {
  using Cfg = Fp8Cfg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bx, by;
  xcd_remap2(bx, by);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // LDS-DMA bases are wave-uniform
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t M = g.M;
  const int K = g.K;
  const int64_t mbase = (int64_t)bx * Cfg::BM;
  const int n0 = by * Cfg::BN;
  const int nk = K / Cfg::KS;

  // staging: instruction j of this wave fills staged rows 8 i .. 8 i + 7, i = wave + 4 j
  // (A rows while i < 16, B rows after); a lane loads the chunk that the swizzle
  // puts at its LDS position
  const uint8_t* ptr[Cfg::LPW];
#pragma unroll
  for (int j = 0; j < Cfg::LPW; ++j) {
    const int i = wave + j * Cfg::NW;
    const int r = (j < Cfg::LPWA ? i : i - Cfg::BM / 8) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ fp8_swz(r);
    if (j < Cfg::LPWA) {
      int64_t gr = mbase + r;
      gr = gr < M ? gr : M - 1;   // tail rows: loaded from the last row, never stored
      ptr[j] = static_cast<const uint8_t*>(g.A) + gr * K + c * 16;
    } else {
      ptr[j] = static_cast<const uint8_t*>(g.B) + (int64_t)(n0 + r) * K + c * 16;
    }
  }
  auto stage = [&](int buf, int ks) __attribute__((always_inline)) {
    GK_LDS char* st = (GK_LDS char*)smem + buf * Cfg::STAGE;
#pragma unroll
    for (int j = 0; j < Cfg::LPW; ++j) glds16(ptr[j] + ks * Cfg::KS, st + (wave + j * Cfg::NW) * 1024);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frag = [&](const char* t, int row) __attribute__((always_inline)) -> i32x8 {
    const char* p = t + row * 128;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(p + ((fq ^ fp8_swz(row)) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(p + (((4 + fq) ^ fp8_swz(row)) << 4));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };

  stage(0, 0);
  for (int t = 0; t < nk; ++t) {
    // slice t has landed for every wave, and every wave is done reading the
    // other stage (slice t - 1), which the next issue overwrites
    vmcnt_le<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) stage((t + 1) & 1, t + 1);
    const char* As = smem + (t & 1) * Cfg::STAGE;
    const char* Bs = As + Cfg::ASTAGE;
    i32x8 bv[4];
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) bv[ns] = frag(Bs, wn * 64 + ns * 16 + fr);
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      const i32x8 av = frag(As, wm * 64 + ms * 16 + fr);
      // weight rows first (e4m3: cbsz 0), activation rows second (blgp AFMT);
      // both scale operands the e8m0 identity, 127
#pragma unroll
      for (int ns = 0; ns < 4; ++ns)
        acc[ms][ns] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bv[ns], av, acc[ms][ns], 0, AFMT, 0,
                                                                       0x7f7f7f7f, 0, 0x7f7f7f7f);
    }
  }

  // epilogue: lane holds C[m = fr][n = 4 fq + r] of every 16 x 16 subtile; lanes fq
  // and fq ^ 1 swap halves of the subtile pair (2 p, 2 p + 1), so each lane owns
  // 8 consecutive columns: one 16-byte store per lane per pair
  const float s = g.sa[0] * g.sb[0];
  const bool odd = fq & 1;
  const int cofs = odd ? 16 + 4 * (fq - 1) : 4 * fq;
  uint16_t* C = static_cast<uint16_t*>(g.C);
  f32x4 bia[4];
#pragma unroll
  for (int ns = 0; ns < 4; ++ns)
    bia[ns] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + n0 + wn * 64 + ns * 16 + 4 * fq)
                     : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ms = 0; ms < 4; ++ms) {
    const int64_t m = mbase + wm * 64 + ms * 16 + fr;
    const bool live = m < M;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float va[4], vb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        va[r] = acc[ms][2 * pr][r] * s + bia[2 * pr][r];
        vb[r] = acc[ms][2 * pr + 1][r] * s + bia[2 * pr + 1][r];
      }
      const uint32_t a0 = pack_bf16x2(va[0], va[1]), a1 = pack_bf16x2(va[2], va[3]);
      const uint32_t b0 = pack_bf16x2(vb[0], vb[1]), b1 = pack_bf16x2(vb[2], vb[3]);
      const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? a0 : b0), 16, 64);
      const uint32_t r1 = (uint32_t)__shfl_xor((int)(odd ? a1 : b1), 16, 64);
      const u32x4 v = odd ? u32x4{r0, r1, b0, b1} : u32x4{a0, a1, r0, r1};
      if (live) *reinterpret_cast<u32x4*>(C + m * g.N + n0 + wn * 64 + pr * 32 + cofs) = v;
    }
  }
}

template <int AFMT>
void launch_gemm_fp8(const Fp8GemmArgs& g, hipStream_t s) {
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_fp8_kernel<AFMT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, Fp8Cfg::LDS) == hipSuccess;
  }();
  (void)attr;
  const int64_t mtiles = (g.M + Fp8Cfg::BM - 1) / Fp8Cfg::BM;
  hipLaunchKernelGGL((gemm_nt_fp8_kernel<AFMT>), dim3((unsigned)mtiles, (unsigned)(g.N / Fp8Cfg::BN)),
                     dim3(Fp8Cfg::THREADS), Fp8Cfg::LDS, s, g);
}

}  // namespace

bool fp8_quant_supported(int64_t R, int64_t C) { return R >= 1 && C >= 16 && C % 16 == 0 && C < (1 << 30); }

void fp8_amax(const Fp8Src& x, uint32_t* partials, hipStream_t s) {
  const int64_t nvec = x.R * x.C / 16;
  if (x.bf16) hipLaunchKernelGGL(fp8_amax_kernel<true>, dim3(fp8_grid(nvec)), dim3(kBlock), 0, s, x.x, nvec, partials);
  else hipLaunchKernelGGL(fp8_amax_kernel<false>, dim3(fp8_grid(nvec)), dim3(kBlock), 0, s, x.x, nvec, partials);
}

void fp8_quantize(const Fp8Src& x, const uint32_t* partials, int fmt, void* q, float* scale, hipStream_t s) {
  const int64_t nvec = x.R * x.C / 16;
  const int grid = fp8_grid(nvec);   // the amax launch's grid: one partial each
#define GK_FP8Q(FMT_, BF_)                                                                                  \
  hipLaunchKernelGGL((fp8_quant_kernel<FMT_, BF_>), dim3(grid), dim3(kBlock), 0, s, x.x, nvec, partials, grid, \
                     static_cast<u32x4*>(q), scale)
  if (fmt == kFp8E4M3) {
    if (x.bf16) GK_FP8Q(kFp8E4M3, true);
    else GK_FP8Q(kFp8E4M3, false);
  } else {
    if (x.bf16) GK_FP8Q(kFp8E5M2, true);
    else GK_FP8Q(kFp8E5M2, false);
  }
#undef GK_FP8Q
}

void fp8_quantize_t(const Fp8Src& w, const uint32_t* partials, void* w8, void* w8t, float* scale, hipStream_t s) {
  const int nparts = fp8_grid(w.R * w.C / 16);
  const dim3 grid((unsigned)((w.C + kQtTile - 1) / kQtTile), (unsigned)((w.R + kQtTile - 1) / kQtTile));
  if (w.bf16)
    hipLaunchKernelGGL(fp8_quant_t_kernel<true>, grid, dim3(kBlock), 0, s, w.x, (int)w.R, (int)w.C, partials, nparts,
                       static_cast<uint8_t*>(w8), static_cast<uint8_t*>(w8t), scale);
  else
    hipLaunchKernelGGL(fp8_quant_t_kernel<false>, grid, dim3(kBlock), 0, s, w.x, (int)w.R, (int)w.C, partials, nparts,
                       static_cast<uint8_t*>(w8), static_cast<uint8_t*>(w8t), scale);
}

bool fp8_gemm_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 128 && K >= 128 && N % 128 == 0 && K % 128 == 0 && N < (1 << 30) && K < (1 << 30) &&
         (M + 127) / 128 < (int64_t)1 << 31 && N / 128 <= 65535;
}

void fp8_gemm_nt(const Fp8GemmArgs& g, hipStream_t s) {
  if (g.afmt == kFp8E4M3) launch_gemm_fp8<kFp8E4M3>(g, s);
  else launch_gemm_fp8<kFp8E5M2>(g, s);
}

}  // namespace gk
