// --------------------------------------------------------------------------
// gemm_tn, fp32 operands: W[N, K] += G[M, N]^T . X[M, K] on v_mfma_f32_16x16x4_f32
// --------------------------------------------------------------------------
// Both operands are M-major (pixel rows), the contraction runs over M, so an
// MFMA operand wants one column of 4 consecutive staged rows per lane.  fp32
// has no transposed LDS read; fp32 MFMA is 16x slower than bf16 per FLOP, so
// 4 ds_read_b32 per 4 MFMAs (128 cycles) cost nothing that matters: lane
// (i = l % 16, g = l / 16) reads rows kb + 4g + j (j = 0..3) of column i and
// MFMA j contracts rows {kb + j, kb + 4 + j, kb + 8 + j, kb + 12 + j} -- the
// same row permutation on both operands.  The 16-byte chunk index of a staged
// row is XOR-ed with bit 2 of the row, which puts the two half-waves of every
// ds_read_b32 (rows 4 apart) on disjoint banks.  Rows past this block's split
// (and padding taps) load from a zero vector, so the tail needs no masking.
// Each wave owns a 64x64 output tile; WN x WK waves per block, ROWS = 32
// pixel rows (two 16-row k-groups, 128 MFMAs per wave) per LDS stage.
#pragma once

#include "gemm_common.h"

namespace gk {
namespace {

__device__ __attribute__((aligned(16))) float g_tn_zero[32];

template <int WN, int WK, int NS_, bool LZ = false>
struct TnF32Cfg {
  static constexpr int NW = WN * WK;
  static constexpr int THREADS = 64 * NW;
  static constexpr int BN = 64 * WN;
  static constexpr int BK = 64 * WK;
  static constexpr int ROWS = 32;
  static constexpr int GROW = BN * 4;
  static constexpr int XROW = BK * 4;
  static constexpr int NGCOPY = LZ ? 2 : 1;        // lazy BN operand: dz and x tiles of G
  static constexpr int GBYTES = ROWS * GROW;       // one G copy
  static constexpr int GBYTES_ALL = NGCOPY * GBYTES;
  static constexpr int STAGE = ROWS * (NGCOPY * GROW + XROW);
  static constexpr int NS = NS_;
  static constexpr int LDS = NS * STAGE;
  static constexpr int GINSTS1 = GBYTES / 1024;
  static constexpr int GINSTS = GBYTES_ALL / 1024;
  static constexpr int INSTS = STAGE / 1024;
  static_assert(INSTS % NW == 0 && GINSTS % NW == 0, "stage split");
  static constexpr int LPW = INSTS / NW;
  static constexpr int LPWG = GINSTS / NW;
  static_assert(LPW <= 63, "wait_vmcnt range");
};

__device__ __forceinline__ int swz4(int r) { return r & 4; }

template <int WN, int WK, int NS, bool GATHER, bool LZ = false, bool X6 = false>
__global__ void __launch_bounds__(64 * WN * WK) __attribute__((amdgpu_waves_per_eu(1)))
gemm_tn_f32_kernel(const float* __restrict__ G, int64_t ldg, const float* __restrict__ X, int64_t ldx,
                   float* __restrict__ W, int64_t ldw, int64_t M, int64_t rows_per_split, ConvGeo geo, LazyA lz) {
  using Cfg = TnF32Cfg<WN, WK, NS, LZ>;
  constexpr int LPW = Cfg::LPW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave % WK, wn = wave / WK;
  int bx, by, bz;   // logical block coordinates (XCD-aware order)
  xcd_remap3(bx, by, bz);
  const int n0 = bx * Cfg::BN;
  const int c0 = by * Cfg::BK;
  const int64_t mbeg = (int64_t)bz * rows_per_split;
  int64_t mend = mbeg + rows_per_split;
  if (mend > M) mend = M;
  if (mbeg >= mend) return;
  const int T = (int)((mend - mbeg + Cfg::ROWS - 1) / Cfg::ROWS);

  // per-lane staging state (set once, advanced by ROWS rows per stage)
  const float* rptr[LPW];
  int64_t row[LPW];
  int pn[LPW], poh[LPW], pow_[LPW], dkh[LPW], dkw[LPW], ccol[LPW];
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    const int i = wave + j * Cfg::NW;
    int srow, colo;
    bool gath = false;
    dkh[j] = dkw[j] = 0;
    if (j < Cfg::LPWG) {
      constexpr int CPR = Cfg::GROW / 16;
      const bool isx = LZ && i >= Cfg::GINSTS1;    // lazy: second G copy = the BN input x
      const int e = (isx ? i - Cfg::GINSTS1 : i) * 64 + lane;
      srow = e / CPR;
      colo = n0 + ((e % CPR) ^ swz4(srow)) * 4;
      rptr[j] = (isx ? static_cast<const float*>(lz.x) : G) + (mbeg + srow) * ldg + colo;
    } else {
      constexpr int CPR = Cfg::XROW / 16;
      const int e = (i - Cfg::GINSTS) * 64 + lane;
      srow = e / CPR;
      const int kcol = c0 + ((e % CPR) ^ swz4(srow)) * 4;
      if (GATHER) {
        const int tap = kcol / geo.C;
        dkh[j] = tap / geo.KW;
        dkw[j] = tap - dkh[j] * geo.KW;
        colo = kcol - tap * geo.C;
        gath = true;
      } else {
        colo = kcol;
      }
      rptr[j] = X + (mbeg + srow) * ldx + colo;
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
      const bool in = row[j] < mend;
      const float* src;
      if (j < Cfg::LPWG) {
        src = in ? rptr[j] : g_tn_zero;
        rptr[j] += gstep;
      } else if (GATHER) {
        const int ih = poh[j] * geo.S - geo.P + dkh[j], iw = pow_[j] * geo.S - geo.P + dkw[j];
        const bool ok = in && (unsigned)ih < (unsigned)geo.H && (unsigned)iw < (unsigned)geo.W;
        const uint32_t off = (((uint32_t)pn[j] * (uint32_t)geo.H + (uint32_t)ih) * (uint32_t)geo.W + (uint32_t)iw) *
                                 (uint32_t)geo.C + (uint32_t)ccol[j];
        src = ok ? X + off : g_tn_zero;
        pow_[j] += adv_r;
        poh[j] += adv_q;
        if (pow_[j] >= geo.OW) { pow_[j] -= geo.OW; ++poh[j]; }
        while (poh[j] >= geo.OH) { poh[j] -= geo.OH; ++pn[j]; }
      } else {
        src = in ? rptr[j] : g_tn_zero;
        rptr[j] += xstep;
      }
      row[j] += Cfg::ROWS;
      glds16(src, base + i * 1024);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane byte offsets of row 4g (+ j + 16 kg: immediates) of this lane's
  // column in each 16-column fragment
  const int fi = lane & 15, fg = lane >> 4;
  int goff[4], xoff[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    const int gc = wn * 64 + s2 * 16 + fi;
    const int xc = wk * 64 + s2 * 16 + fi;
    const int r = 4 * fg;
    goff[s2] = r * Cfg::GROW + ((((gc >> 2) ^ swz4(r)) << 4) | ((gc & 3) << 2));
    xoff[s2] = Cfg::GBYTES_ALL + r * Cfg::XROW + ((((xc >> 2) ^ swz4(r)) << 4) | ((xc & 3) << 2));
  }
  // lazy operand: coefficients of this lane's four G columns (fixed for the block)
  float4 cf[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2)
    cf[s2] = LZ ? reinterpret_cast<const float4*>(lz.coef)[n0 + wn * 64 + s2 * 16 + fi] : make_float4(0.f, 0.f, 0.f, 0.f);

  stage(0);
  if (NS >= 3 && T > 1) stage(1);
  for (int t = 0; t < T; ++t) {
    if (NS == 3) wait_vmcnt_fast<LPW>(t + 1 < T ? LPW : 0);
    else wait_vmcnt(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + NS - 1 < T) stage(t + NS - 1);
    const char* sb = smem + (t % NS) * Cfg::STAGE;
    const int64_t mst = mbeg + (int64_t)t * Cfg::ROWS;   // first row of this stage
    const bool tail = LZ && mst + Cfg::ROWS > mend;      // lazy: rows past the split must give 0, not k1(-k2 + mu k4)
    // fragments of k-group kg: [j][s2] (32 values); the next group's reads are
    // issued before this group's 64 MFMAs so only one LDS latency per stage shows
    float gv[2][4][4], xv[2][4][4];
    auto load = [&](int kg, float (&g)[4][4], float (&x)[4][4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rr = kg * 16 + j;   // row offset of MFMA j's k-slot 0
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
          g[j][s2] = *reinterpret_cast<const float*>(sb + goff[s2] + rr * Cfg::GROW);
          x[j][s2] = *reinterpret_cast<const float*>(sb + xoff[s2] + rr * Cfg::XROW);
        }
        if constexpr (LZ) {
          const bool live = !tail || mst + rr + 4 * fg < mend;
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) {
            const float xz = *reinterpret_cast<const float*>(sb + Cfg::GBYTES + goff[s2] + rr * Cfg::GROW);
            const float d = cf[s2].x * ((g[j][s2] - cf[s2].y) - (xz - cf[s2].z) * cf[s2].w);
            g[j][s2] = live ? d : 0.f;
          }
        }
      }
    };
    if constexpr (X6) {
      // bf16x6 products (gemm_nt_kernel X6): the lane's 8 rows {16 kg + 4 fg + j}
      // of a column form one 16x16x32 bf16 operand (the same row permutation on
      // G and X), split exactly into hi + mid + lo parts
      load(0, gv[0], xv[0]);
      load(1, gv[1], xv[1]);
      bf16x8 gh[4], gm[4], gl[4];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
        split3x8(f32x4{gv[0][0][s2], gv[0][1][s2], gv[0][2][s2], gv[0][3][s2]},
                 f32x4{gv[1][0][s2], gv[1][1][s2], gv[1][2][s2], gv[1][3][s2]}, gh[s2], gm[s2], gl[s2]);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 xh, xm, xl;
        split3x8(f32x4{xv[0][0][ks], xv[0][1][ks], xv[0][2][ks], xv[0][3][ks]},
                 f32x4{xv[1][0][ks], xv[1][1][ks], xv[1][2][ks], xv[1][3][ks]}, xh, xm, xl);
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
          f32x4 c = acc[ns][ks];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gl[ns], xh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gh[ns], xl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gm[ns], xm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gm[ns], xh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gh[ns], xm, c, 0, 0, 0);
          acc[ns][ks] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gh[ns], xh, c, 0, 0, 0);
        }
      }
      continue;
    }
    load(0, gv[0], xv[0]);
#pragma unroll
    for (int kg = 0; kg < Cfg::ROWS / 16; ++kg) {
      if (kg + 1 < Cfg::ROWS / 16) load(kg + 1, gv[(kg + 1) & 1], xv[(kg + 1) & 1]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ns = 0; ns < 4; ++ns)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            acc[ns][ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[kg & 1][j][ns], xv[kg & 1][j][ks], acc[ns][ks], 0, 0, 0);
    }
  }
  // D[i = n][j = c]: lane holds column c = .. + (lane & 15), rows n = .. + 4 (lane >> 4) + r
#pragma unroll
  for (int ns = 0; ns < 4; ++ns)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int c = c0 + wk * 64 + ks * 16 + fi;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn * 64 + ns * 16 + fg * 4 + r;
        atomicAdd(W + (int64_t)n * ldw + c, acc[ns][ks][r]);
      }
    }
}

template <int WN, int WK, int NS, bool GATHER, bool LZ = false, bool X6 = false>
void launch_tn_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw, int64_t M, int N,
                   int K, int splits, const ConvGeo& geo, const LazyA& lz, hipStream_t stream) {
  using Cfg = TnF32Cfg<WN, WK, NS, LZ>;
  const int tiles = (N / Cfg::BN) * (K / Cfg::BK);
  if (splits <= 0) {
    // two rounds of the chip's block slots (LDS-limited blocks per CU)
    static const int cus = [] {
      int d = 0, n = 0;
      hipGetDevice(&d);
      return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0 ? n : 256;
    }();
    int bpc = (160 * 1024) / Cfg::LDS;
    const int by_waves = 16 / Cfg::NW;
    if (bpc > by_waves) bpc = by_waves;
    if (bpc < 1) bpc = 1;
    // splits < 0: -splits quarter rounds (see launch_tn); 0: two rounds
    const int64_t quarters = splits == 0 ? 8 : -(int64_t)splits;
    splits = (int)(quarters * (int64_t)cus * bpc / (4 * (int64_t)tiles));
    if (splits < 1) splits = 1;
  }
  int64_t rows = (M + splits - 1) / splits;
  rows = (rows + Cfg::ROWS - 1) / Cfg::ROWS * Cfg::ROWS;
  if (rows < 4 * Cfg::ROWS) rows = 4 * Cfg::ROWS;
  const int64_t nsplit = (M + rows - 1) / rows;
  dim3 grid((unsigned)(N / Cfg::BN), (unsigned)(K / Cfg::BK), (unsigned)nsplit);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_f32_kernel<WN, WK, NS, GATHER, LZ, X6>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL((gemm_tn_f32_kernel<WN, WK, NS, GATHER, LZ, X6>), grid, dim3(Cfg::THREADS), Cfg::LDS, stream, G, ldg,
                     X, ldx, W, ldw, M, rows, geo, lz);
}

// Reaches the instantiations that cfg::tn_f32_select can name (gemm_cfg.h: tiles, fallbacks);
// a three-stage request is kept where the tile's LDS fits.
template <bool GATHER, bool X6 = false>
void tn_f32_dispatch(const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw, int64_t M, int N,
                     int K, const cfg::TnF32Word& w, int splits, const ConvGeo& geo, const LazyArgs* lza,
                     hipStream_t stream) {
  const cfg::TnF32Sel s = cfg::tn_f32_select(w, N, K, lza != nullptr);
  const bool ns3 = s.stages == 3;
  const LazyA lz = lza ? LazyA{lza->x, lza->coef, lza->padz, lza->padx, lza->C} : LazyA{};
#define GK_TNL(WN_, WK_, LZ_)                                                                                   \
  do {                                                                                                          \
    if (ns3 && TnF32Cfg<WN_, WK_, 3, LZ_>::LDS <= 160 * 1024)                                                   \
      launch_tn_f32<WN_, WK_, 3, GATHER, LZ_, X6>(G, ldg, X, ldx, W, ldw, M, N, K, splits, geo, lz, stream);     \
    else                                                                                                        \
      launch_tn_f32<WN_, WK_, 2, GATHER, LZ_, X6>(G, ldg, X, ldx, W, ldw, M, N, K, splits, geo, lz, stream);     \
  } while (0)
#define GK_TNF(WN_, WK_)              \
  case cfg::tn_f32_key(WN_, WK_):     \
    if (s.lz) GK_TNL(WN_, WK_, true); \
    else GK_TNL(WN_, WK_, false);     \
    break
  switch (cfg::tn_f32_key(s.wn, s.wk)) {
    GK_TNF(2, 1);
    GK_TNF(1, 2);
    GK_TNF(2, 2);
    GK_TNF(4, 1);
    GK_TNF(1, 4);
    GK_TNF(4, 2);
    GK_TNF(2, 4);
    case cfg::tn_f32_key(4, 4): GK_TNL(4, 4, false); break;   // no lazy 256x256 tile: it does not fit in LDS
    GK_TNF(1, 1);
  }
#undef GK_TNF
#undef GK_TNL
}

}  // namespace
}  // namespace gk
