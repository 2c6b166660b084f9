// gemm_tn: reduction over the pixel dimension M; both operands are
//   M-major, so fragments are read with ds_read_b64_tr_b16 (the gfx950 LDS
//   transpose read: 4 rows x 16 columns of 16-bit data delivered column-wise).
//   Each block reduces a contiguous slice of M for one output tile and adds
//   its fp32 partial into the (gradient-arena) output with float atomics.
#pragma once

#include "gemm_common.h"

namespace gk {
namespace {

// --------------------------------------------------------------------------
// gemm_tn: W[N, K] += G[M, N]^T . X[M, K]
// --------------------------------------------------------------------------
// WS waves split the 64*WS pixel rows of a stage for the same output tile;
// their partial sums are combined through LDS before the atomics.
// MSN: 64-row groups of the wave tile along N (1: 64x64 per wave, 2: 128x64 --
// 25% fewer LDS reads per MFMA and twice the work per staged G row)
template <int WN, int WK, int WS, int NS_, int MSN = 1>
struct TnCfg {
  static constexpr int NW = WN * WK * WS;
  static constexpr int THREADS = 64 * NW;
  static constexpr int WTN = 64 * MSN;               // wave tile rows (G columns)
  static constexpr int BN = WTN * WN;                // output rows (G columns)
  static constexpr int BK = 64 * WK;                 // output cols (X columns)
  static constexpr int ROWS = 64 * WS;               // pixel rows per stage
  static constexpr int GROW = BN * 2;                // bytes per staged G row
  static constexpr int XROW = BK * 2;
  static constexpr int GBYTES = ROWS * GROW;
  static constexpr int STAGE = ROWS * (GROW + XROW);
  static constexpr int NS = NS_;                     // LDS stages (3: two slices in flight)
  static constexpr int LDS = NS * STAGE;
  static constexpr int GINSTS = GBYTES / 1024;
  static constexpr int INSTS = STAGE / 1024;
  static_assert(INSTS % NW == 0, "stage split");
  static constexpr int LPW = INSTS / NW;
  static_assert(LPW <= 63, "wait_vmcnt range");
  static_assert(GINSTS % NW == 0, "G rows split evenly over the waves");
  static constexpr int LPWG = GINSTS / NW;           // G-row instructions per wave (j < LPWG)
  static_assert((WS - 1) * WN * WK * MSN * 16384 <= LDS, "reduction scratch");
};

// The transposed LDS reads are issued as inline asm: with the builtin, the
// compiler's wait-count pass cannot tell the read apart from the LDS-DMA
// writes of the NEXT stage issued just before it and inserts `s_waitcnt
// vmcnt(0)` -- which serialises the whole global->LDS pipeline (each stage
// would wait for the loads it has just started).  The asm reads carry no such
// dependence; tr_sync() below waits for them (lgkmcnt) and ties the fragments
// to that wait so no MFMA can be scheduled before it.
//
// tr_pair: the two halves of a transposed fragment at precomputed LDS
// addresses, k-step kk adding the immediate kk * KSTEP bytes
template <int KSTEP>
__device__ __forceinline__ bf16x8 tr_pair(uint32_t a0, uint32_t a1, int kk) {
  bf16x4 lo, hi;
  if (kk == 0) {
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(a1));
  } else {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(a0), "i"(KSTEP));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(a1), "i"(KSTEP));
  }
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// lgkmcnt(0) tied to the fragments of one k-step
template <int MSN>
__device__ __forceinline__ void tr_sync(bf16x8* a, bf16x8* b) {
  if (MSN == 1) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                   "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  }
}

template <int WN, int WK, int WS, int NS, bool GATHER, int MSN = 1>
__global__ void __launch_bounds__(64 * WN * WK * WS) __attribute__((amdgpu_waves_per_eu(MSN > 1 ? 1 : 2)))
gemm_tn_kernel(const uint16_t* __restrict__ G, int64_t ldg, const uint16_t* __restrict__ X, int64_t ldx,
               float* __restrict__ W, int64_t ldw, int64_t M, int64_t rows_per_split, ConvGeo geo) {
  using Cfg = TnCfg<WN, WK, WS, NS, MSN>;
  constexpr int NF = 4 * MSN;                        // G fragments (16 rows each) per wave
  constexpr int LPW = Cfg::LPW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wk = wave % WK, wn = (wave / WK) % WN, ws = wave / (WK * WN);
  int bx, by, bz;   // logical block coordinates (XCD-aware order)
  xcd_remap3(bx, by, bz);
  const int n0 = bx * Cfg::BN;
  const int c0 = by * Cfg::BK;
  const int64_t mbeg = (int64_t)bz * rows_per_split;
  int64_t mend = mbeg + rows_per_split;
  if (mend > M) mend = M;
  if (mbeg >= mend) return;
  const int T = (int)((mend - mbeg + Cfg::ROWS - 1) / Cfg::ROWS);

  // Per-lane staging state, set up once and advanced by ROWS pixel rows per
  // stage (no per-stage divisions or 64-bit multiplies): G / plain-X
  // instructions keep a row pointer; gathered X instructions keep the output
  // pixel (n, oh, ow) and their tap (dkh, dkw).
  const uint16_t* rptr[LPW];     // current row pointer (G / plain X)
  const uint16_t* rlast[LPW];    // row M-1 (clamp target past the end)
  int64_t row[LPW];              // current pixel row index
  int pn[LPW], poh[LPW], pow_[LPW], dkh[LPW], dkw[LPW], ccol[LPW];
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    const int i = wave + j * Cfg::NW;
    int srow, colo;
    bool gath = false;
    dkh[j] = dkw[j] = 0;
    if (j < Cfg::LPWG) {
      constexpr int CPR = Cfg::GROW / 16;
      const int e = i * 64 + lane;
      srow = e / CPR;
      colo = n0 + ((e % CPR) ^ tr_swz<Cfg::GROW>(srow)) * 8;
      rptr[j] = G + (mbeg + srow) * ldg + colo;
      rlast[j] = G + (M - 1) * ldg + colo;
    } else {
      constexpr int CPR = Cfg::XROW / 16;
      const int e = (i - Cfg::GINSTS) * 64 + lane;
      srow = e / CPR;
      const int ch = (e % CPR) ^ tr_swz<Cfg::XROW>(srow);
      if (GATHER) {
        const int k0 = c0 + (ch >> 3) * 64;          // 64-channel slice of one tap
        const int tap = k0 / geo.C;
        dkh[j] = tap / geo.KW;
        dkw[j] = tap - dkh[j] * geo.KW;
        colo = (k0 - tap * geo.C) + (ch & 7) * 8;
        gath = true;
      } else {
        colo = c0 + ch * 8;
      }
      rptr[j] = X + (mbeg + srow) * ldx + colo;
      rlast[j] = X + (M - 1) * ldx + colo;
    }
    row[j] = mbeg + srow;
    ccol[j] = colo;
    pn[j] = poh[j] = pow_[j] = 0;
    if (GATHER && gath) {
      const int64_t m = mbeg + srow;
      const int64_t ohw = (int64_t)geo.OH * geo.OW;
      pn[j] = (int)(m / ohw);
      const int rem = (int)(m - (int64_t)pn[j] * ohw);
      poh[j] = rem / geo.OW;
      pow_[j] = rem - poh[j] * geo.OW;
    }
  }
  const int adv_q = Cfg::ROWS / (GATHER ? geo.OW : 1), adv_r = Cfg::ROWS - adv_q * (GATHER ? geo.OW : 1);
  const int64_t gstep = (int64_t)Cfg::ROWS * ldg, xstep = (int64_t)Cfg::ROWS * ldx;

  auto stage = [&](int t) {
    GK_LDS char* base = (GK_LDS char*)smem + (t % NS) * Cfg::STAGE;
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int i = wave + j * Cfg::NW;
      const bool in = row[j] < M;
      const uint16_t* src;
      if (j < Cfg::LPWG) {
        src = in ? rptr[j] : rlast[j];
        rptr[j] += gstep;
      } else if (GATHER) {
        const int ih = poh[j] * geo.S - geo.P + dkh[j], iw = pow_[j] * geo.S - geo.P + dkw[j];
        const bool ok = in && (unsigned)ih < (unsigned)geo.H && (unsigned)iw < (unsigned)geo.W;
        const uint32_t off = (((uint32_t)pn[j] * (uint32_t)geo.H + (uint32_t)ih) * (uint32_t)geo.W + (uint32_t)iw) *
                                 (uint32_t)geo.C + (uint32_t)ccol[j];
        src = ok ? X + off : static_cast<const uint16_t*>(geo.zero) + (ccol[j] & 63);
        // advance the pixel by ROWS
        pow_[j] += adv_r;
        poh[j] += adv_q;
        if (pow_[j] >= geo.OW) { pow_[j] -= geo.OW; ++poh[j]; }
        while (poh[j] >= geo.OH) { poh[j] -= geo.OH; ++pn[j]; }
      } else {
        src = in ? rptr[j] : rlast[j];
        rptr[j] += xstep;
      }
      row[j] += Cfg::ROWS;
      glds16(src, base + i * 1024);
    }
  };

  f32x4 acc[NF][4];
#pragma unroll
  for (int a = 0; a < NF; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Per-lane LDS byte offsets of the 16 transposed reads of a k-step, set up
  // once: the swizzle depends on row bits 0, 1 and 3 only, so the second
  // k-step (rows + 32) is the same addresses + 32 rows -- an immediate offset
  // -- and a new stage only adds its (uniform) base: 16 adds per stage instead
  // of the full address arithmetic per read.
  uint32_t goff[NF][2], xoff[4][2];
  {
    const int g = lane >> 4, li = lane & 15;
    const int q = li >> 2, p = li & 3;
    const int ra = ws * 64 + 8 * g + q, rb = ra + 4;
#pragma unroll
    for (int s2 = 0; s2 < NF; ++s2) {
      const int gc = wn * Cfg::WTN + s2 * 16 + 4 * p;
      goff[s2][0] = ra * Cfg::GROW + ((((gc >> 3) ^ tr_swz<Cfg::GROW>(ra)) << 4) | ((gc & 7) << 1));
      goff[s2][1] = rb * Cfg::GROW + ((((gc >> 3) ^ tr_swz<Cfg::GROW>(rb)) << 4) | ((gc & 7) << 1));
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const int xc = wk * 64 + s2 * 16 + 4 * p;
      xoff[s2][0] = Cfg::GBYTES + ra * Cfg::XROW + ((((xc >> 3) ^ tr_swz<Cfg::XROW>(ra)) << 4) | ((xc & 7) << 1));
      xoff[s2][1] = Cfg::GBYTES + rb * Cfg::XROW + ((((xc >> 3) ^ tr_swz<Cfg::XROW>(rb)) << 4) | ((xc & 7) << 1));
    }
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)(GK_LDS char*)smem;

  stage(0);
  if (NS == 3 && T > 1) stage(1);
  for (int t = 0; t < T; ++t) {
    // retire slice t (with NS = 3, slice t+1 stays in flight)
    if (NS == 3) wait_vmcnt_fast<LPW>(t + 1 < T ? LPW : 0);
    else wait_vmcnt(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + NS - 1 < T) stage(t + NS - 1);
    const uint32_t sb = lds0 + (uint32_t)((t % NS) * Cfg::STAGE);
    uint32_t ga[NF][2], xa[4][2];
#pragma unroll
    for (int s2 = 0; s2 < NF; ++s2)
#pragma unroll
      for (int h = 0; h < 2; ++h) ga[s2][h] = sb + goff[s2][h];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int h = 0; h < 2; ++h) xa[s2][h] = sb + xoff[s2][h];
    const int64_t m0 = mbeg + (int64_t)t * Cfg::ROWS + ws * 64;
    const bool tail = m0 + 64 > mend;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 gv[NF], xv[4];
#pragma unroll
      for (int s2 = 0; s2 < NF; ++s2) gv[s2] = tr_pair<32 * Cfg::GROW>(ga[s2][0], ga[s2][1], kk);
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) xv[s2] = tr_pair<32 * Cfg::XROW>(xa[s2][0], xa[s2][1], kk);
      tr_sync<MSN>(gv, xv);
      if (tail) {  // rows past this split's end contribute nothing
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int64_t m = m0 + kk * 32 + 8 * (lane >> 4) + j;
          if (m >= mend) {
#pragma unroll
            for (int s2 = 0; s2 < NF; ++s2) gv[s2][j] = 0;
          }
        }
      }
#pragma unroll
      for (int ns = 0; ns < NF; ++ns)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          acc[ns][ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gv[ns], xv[ks], acc[ns][ks], 0, 0, 0);
    }
  }
  if (WS > 1) {   // combine the WS partial tiles through LDS
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    const int slot = wn * WK + wk;
    if (ws > 0) {
#pragma unroll
      for (int ns = 0; ns < NF; ++ns)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          red[(((ws - 1) * WN * WK + slot) * 4 * NF + ns * 4 + ks) * 64 + lane] = acc[ns][ks];
    }
    __syncthreads();
    if (ws == 0) {
#pragma unroll
      for (int w2 = 1; w2 < WS; ++w2)
#pragma unroll
        for (int ns = 0; ns < NF; ++ns)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const f32x4 v = red[(((w2 - 1) * WN * WK + slot) * 4 * NF + ns * 4 + ks) * 64 + lane];
            acc[ns][ks] += v;
          }
    }
  }
  if (ws != 0) return;
  // D[i = n][j = c]: lane holds column c = .. + (lane&15), rows n = .. + 4*(lane>>4) + r
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int ns = 0; ns < NF; ++ns)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int c = c0 + wk * 64 + ks * 16 + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn * Cfg::WTN + ns * 16 + fq * 4 + r;
        atomicAdd(W + (int64_t)n * ldw + c, acc[ns][ks][r]);
      }
    }
}

template <int WN, int WK, int WS, int NS, bool GATHER, int MSN = 1>
void launch_tn(const uint16_t* G, int64_t ldg, const uint16_t* X, int64_t ldx, float* W, int64_t ldw, int64_t M,
               int N, int K, int splits, const ConvGeo& geo, hipStream_t stream) {
  using Cfg = TnCfg<WN, WK, WS, NS, MSN>;
  const int tiles = (N / Cfg::BN) * (K / Cfg::BK);
  if (splits <= 0) {
    // Whole rounds of the chip: one 8-wave block per CU at 2 waves / SIMD
    // (the 16-wave tile: one per CU too), two rounds -- a 2.1-round grid
    // would leave the third round almost empty (a 33% tail).
    static const int cus = [] {
      int d = 0, n = 0;
      hipGetDevice(&d);
      return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0 ? n : 256;
    }();
    const int64_t bpc = Cfg::NW >= 8 ? 1 : 8 / Cfg::NW;
    const int64_t slots = (int64_t)cus * bpc;
    // splits < 0: -splits quarter rounds (a grad-weight on the side stream that
    // should leave CUs to the critical path); 0: two rounds
    const int64_t quarters = splits == 0 ? 8 : -(int64_t)splits;
    splits = (int)(quarters * slots / (4 * (int64_t)tiles));
    if (splits < 1) splits = 1;
  }
  int64_t rows = (M + splits - 1) / splits;
  rows = (rows + Cfg::ROWS - 1) / Cfg::ROWS * Cfg::ROWS;
  if (rows < 4 * Cfg::ROWS) rows = 4 * Cfg::ROWS;
  const int64_t nsplit = (M + rows - 1) / rows;
  dim3 grid((unsigned)(N / Cfg::BN), (unsigned)(K / Cfg::BK), (unsigned)nsplit);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_kernel<WN, WK, WS, NS, GATHER, MSN>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL((gemm_tn_kernel<WN, WK, WS, NS, GATHER, MSN>), grid, dim3(Cfg::THREADS), Cfg::LDS, stream, G, ldg, X, ldx, W, ldw,
                     M, rows, geo);
}

template <int WN, int WK, int WS, bool GATHER, int MSN = 1>
void launch_tn_any(const uint16_t* G, int64_t ldg, const uint16_t* X, int64_t ldx, float* W, int64_t ldw, int64_t M,
                   int N, int K, int splits, int ns, const ConvGeo& geo, hipStream_t stream) {
  if (ns == 3 && TnCfg<WN, WK, WS, 3, MSN>::LDS <= 160 * 1024)
    launch_tn<WN, WK, WS, 3, GATHER, MSN>(G, ldg, X, ldx, W, ldw, M, N, K, splits, geo, stream);
  else launch_tn<WN, WK, WS, 2, GATHER, MSN>(G, ldg, X, ldx, W, ldw, M, N, K, splits, geo, stream);
}

// Reaches the instantiations that cfg::tn_select can name (gemm_cfg.h: tiles, fallbacks).
// 128x64 per wave (MSN 2, one wave per SIMD to fit 340-460 VGPRs) measured 1.3-3x slower than
// the 64x64 tiles on every BERT / ResNet-50 grad-weight shape (profiles/r02_tn_probe.json), so
// no tile instantiates it; the template parameter stays for future occupancy experiments.
template <bool GATHER>
void tn_dispatch(const void* G, int64_t ldg, const void* X, int64_t ldx, float* W, int64_t ldw, int64_t M, int N,
                 int K, const cfg::TnWord& w, int splits, const ConvGeo& geo, hipStream_t stream) {
  auto g = static_cast<const uint16_t*>(G);
  auto x = static_cast<const uint16_t*>(X);
  const cfg::TnSel s = cfg::tn_select(w, N, K);
#define GK_TN(WN_, WK_, WS_)           \
  case cfg::tn_key(WN_, WK_, WS_):     \
    launch_tn_any<WN_, WK_, WS_, GATHER>(g, ldg, x, ldx, W, ldw, M, N, K, splits, s.stages, geo, stream); \
    break
  switch (cfg::tn_key(s.wn, s.wk, s.ws)) {
    GK_TN(4, 2, 1);
    GK_TN(2, 4, 1);
    GK_TN(4, 4, 1);
    GK_TN(2, 1, 2);
    GK_TN(1, 2, 2);
    GK_TN(2, 2, 1);
    GK_TN(4, 1, 1);
    GK_TN(1, 4, 1);
    GK_TN(2, 2, 2);
    GK_TN(1, 1, 2);
    GK_TN(1, 1, 4);
  }
#undef GK_TN
}

}  // namespace
}  // namespace gk
