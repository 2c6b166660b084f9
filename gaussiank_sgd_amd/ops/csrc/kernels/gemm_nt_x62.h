// --------------------------------------------------------------------------
// gemm_nt, bf16x6 with register staging ("x62"): C[M, N] = A[M, K] B[N, K]^T,
// fp32 operands, row GEMMs only
// --------------------------------------------------------------------------
// The X6 form of gemm_nt_kernel stages fp32 tiles by LDS-DMA and every wave
// splits the fragments it reads, so each element is split once per wave that
// reads it (twice on a 2x2 wave grid) and every 1 KiB of fp32 costs one
// LDS-DMA issue (~60-185 cycles among MFMAs, MI355X_MICROARCH.md).  Here
// each thread loads 8 consecutive K elements of a row pair-wise into
// registers (global_load_dwordx4), splits them ONCE (split3x8) and writes the
// three bf16 planes to LDS; the MFMA loop reads bf16 fragments directly.  The
// next slice's loads are in flight during the current slice's MFMAs and its
// split + LDS writes are issued in the middle of them (two LDS stages of
// 3 x (BM + BN) x 64 bytes, one barrier per 32-deep K slice).  Persistent over
// M tiles like gemm_nt_kernel; XCD-aware block order; epilogue: bias, the
// BatchNorm statistics partials or the BN-backward dz (fp32 layouts of
// gemm_nt_kernel).
#pragma once

#include "gemm_common.h"

namespace gk {
namespace {

template <int WM, int WN>
struct X62Cfg {
  static constexpr int NW = WM * WN;
  static constexpr int THREADS = 64 * NW;
  static constexpr int BM = 64 * WM;
  static constexpr int BN = 64 * WN;
  static constexpr int PA = BM * 64;                 // bytes of one A plane (BM rows x 32 bf16)
  static constexpr int PB = BN * 64;
  static constexpr int STAGE = 3 * (PA + PB);
  static constexpr int LDS = 2 * STAGE;
  static constexpr int PRA = BM * 4 / THREADS;       // 8-element row pieces of A per thread per slice
  static constexpr int PRB = BN * 4 / THREADS;
  static_assert(PRA >= 1 && PRB >= 1 && (BM * 4) % THREADS == 0 && (BN * 4) % THREADS == 0, "pieces per thread");
  static_assert(LDS <= 160 * 1024, "LDS");
};

// D2C (with BNB, row GEMMs): the BN-backward epilogue's dy2 is compact (BnBwd OW > 0)
template <int WM, int WN, bool BNB, int NPF = 1, bool GATHER = false, bool P3 = false, bool D2C = false>
__global__ void __launch_bounds__(64 * WM * WN) __attribute__((amdgpu_waves_per_eu(1)))
gemm_nt_x62_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                   float* __restrict__ C, int64_t ldc, int64_t M, int K, const float* __restrict__ bias,
                   float* __restrict__ stats, int64_t stats_ld, BnBwd bb, ConvGeo geo) {
  // GATHER: implicit-GEMM convolution over channels-last A = x [N, H, W, C]
  // (gemm_nt_kernel's ConvGeo, C a multiple of 32): row m is output pixel
  // (n, oh, ow), K slice ks is tap (kh, kw) of channels c0 .. c0 + 31; a tap
  // outside the image loads geo.zero
  using Cfg = X62Cfg<WM, WN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bx, by;
  xcd_remap2(bx, by);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = by * Cfg::BN;
  const int Ntot = (int)gridDim.y * Cfg::BN;
  const int64_t mtiles = (M + Cfg::BM - 1) / Cfg::BM;
  const int nk = K / 32;
  const int64_t my_tiles = bx < mtiles ? (mtiles - 1 - bx) / gridDim.x + 1 : 0;
  const int T_ = (int)(my_tiles * nk);
  if (T_ == 0) {
    if (stats)
      for (int c = tid; c < Cfg::BN; c += Cfg::THREADS) {
        stats[(int64_t)bx * Ntot + n0 + c] = 0.f;
        stats[stats_ld + (int64_t)bx * Ntot + n0 + c] = 0.f;
      }
    return;
  }

  // ---- register staging: piece p of A is row cid >> 2, K elements 8 (cid & 3) .. +7
  // of the slice (cid = tid + THREADS p); same for B (rows of the weight panel)
  // NPF register sets: the loads of slice s go to set s % NPF (NPF = 2: two
  // slices in flight ahead of the one being multiplied)
  // P3: B arrives pre-split (geo.b3, [N][K/32][3][32] bf16): a B piece is three
  // 16-byte loads written to the planes as they are -- no split VALU for B
  f32x4 ra[NPF][Cfg::PRA][2], rb[NPF][P3 ? 1 : Cfg::PRB][2];
  u32x4 rb3[NPF][P3 ? Cfg::PRB : 1][3];
  const uint16_t* lpb3[P3 ? Cfg::PRB : 1];
  // load cursor: per-piece pointers to the next slice's 8 floats, advanced by
  // 32 floats per slice; the 64-bit row arithmetic runs only at an M-tile
  // change (a wave-uniform branch), not for every slice
  int64_t l_mt = bx;
  int l_ks = 0;
  const float* lpa[GATHER ? 1 : Cfg::PRA];
  const float* lpb[Cfg::PRB];
  // gather: tap / channel offset of the next slice (wave-uniform) and, per
  // piece, its output pixel's in-image taps (bits kh of okhw, bits 8 + kw) and
  // its 32-bit element offset into x (the host refuses x of >= 2^31 elements):
  // two registers per piece instead of four -- the 4x2-wave gather tiles
  // spilled with 64-bit pointers and separate tap masks
  int l_kh = 0, l_kw = 0, l_c0 = 0;
  uint32_t okhw[GATHER ? Cfg::PRA : 1];
  int32_t aoff[GATHER ? Cfg::PRA : 1];
  auto set_a_rows = [&]() __attribute__((always_inline)) {
    const int64_t m0 = l_mt * Cfg::BM;
#pragma unroll
    for (int p = 0; p < Cfg::PRA; ++p) {
      const int cid = tid + Cfg::THREADS * p;
      int64_t gr = m0 + (cid >> 2);
      gr = gr < M ? gr : M - 1;   // tail rows: computed, never stored
      if constexpr (GATHER) {
        const uint32_t ohw = (uint32_t)(geo.OH * geo.OW);
        const uint32_t mu = (uint32_t)gr;
        const uint32_t n = mu / ohw, rem = mu - n * ohw;
        const uint32_t oh = rem / (uint32_t)geo.OW, ow = rem - oh * (uint32_t)geo.OW;
        const int ih0 = (int)oh * geo.S - geo.P, iw0 = (int)ow * geo.S - geo.P;
        uint32_t bh = 0u, bw = 0u;
#pragma unroll
        for (int t = 0; t < kMaxTaps; ++t) {
          bh |= (uint32_t)((unsigned)(ih0 + t) < (unsigned)geo.H) << t;
          bw |= (uint32_t)((unsigned)(iw0 + t) < (unsigned)geo.W) << t;
        }
        okhw[p] = bh | (bw << 8);
        aoff[p] = (((int)n * geo.H + ih0) * geo.W + iw0) * geo.C + (cid & 3) * 8;
      } else {
        lpa[p] = A + gr * lda + (cid & 3) * 8;
      }
    }
  };
  set_a_rows();
#pragma unroll
  for (int p = 0; p < Cfg::PRB; ++p) {
    const int cid = tid + Cfg::THREADS * p;
    if constexpr (P3) lpb3[p] = geo.b3 + (int64_t)(n0 + (cid >> 2)) * (3 * K) + (cid & 3) * 8;
    else lpb[p] = B + (int64_t)(n0 + (cid >> 2)) * ldb + (cid & 3) * 8;
  }
  const float* zrow = static_cast<const float*>(geo.zero);
  auto issue_loads = [&](auto SET) __attribute__((always_inline)) {
    constexpr int q = decltype(SET)::value;
    const int64_t toff = GATHER ? (int64_t)(l_kh * geo.W + l_kw) * geo.C + l_c0 : 0;   // wave-uniform
#pragma unroll
    for (int p = 0; p < Cfg::PRA; ++p) {
      const float* src;
      if constexpr (GATHER) {
        const bool ok = ((okhw[p] >> l_kh) & (okhw[p] >> (8 + l_kw)) & 1u) != 0u;
        src = ok ? A + ((int64_t)aoff[p] + toff) : zrow;
      } else {
        src = lpa[p];
        lpa[p] += 32;
      }
      ra[q][p][0] = *reinterpret_cast<const f32x4*>(src);
      ra[q][p][1] = *reinterpret_cast<const f32x4*>(src + 4);
    }
#pragma unroll
    for (int p = 0; p < Cfg::PRB; ++p) {
      if constexpr (P3) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) rb3[q][p][pl] = *reinterpret_cast<const u32x4*>(lpb3[p] + pl * 32);
        lpb3[p] += 96;
      } else {
        rb[q][p][0] = *reinterpret_cast<const f32x4*>(lpb[p]);
        rb[q][p][1] = *reinterpret_cast<const f32x4*>(lpb[p] + 4);
        lpb[p] += 32;
      }
    }
    if constexpr (GATHER) {
      l_c0 += 32;
      if (l_c0 == geo.C) {
        l_c0 = 0;
        if (++l_kw == geo.KW) {
          l_kw = 0;
          ++l_kh;
        }
      }
    }
    if (++l_ks == nk) {
      l_ks = 0;
      l_kh = l_kw = l_c0 = 0;
      l_mt += gridDim.x;
      set_a_rows();
#pragma unroll
      for (int p = 0; p < Cfg::PRB; ++p) {
        if constexpr (P3) lpb3[p] -= 3 * K;
        else lpb[p] -= K;
      }
    }
  };
  // piece pc of the slice (A pieces 0 .. PRA-1, then B pieces), or all of them (pc < 0)
  auto split_write = [&](int buf, auto SET, int pc = -1) __attribute__((always_inline)) {
    constexpr int q = decltype(SET)::value;
    char* st = smem + buf * Cfg::STAGE;
#pragma unroll
    for (int p = 0; p < Cfg::PRA; ++p) {
      if (pc >= 0 && pc != p) continue;
      const int cid = tid + Cfg::THREADS * p;
      const int r = cid >> 2;
      bf16x8 h, m, l;
      split3x8(ra[q][p][0], ra[q][p][1], h, m, l);
      const int off = r * 64 + (((cid & 3) ^ x62_swz(r)) << 4);
      *reinterpret_cast<bf16x8*>(st + off) = h;
      *reinterpret_cast<bf16x8*>(st + Cfg::PA + off) = m;
      *reinterpret_cast<bf16x8*>(st + 2 * Cfg::PA + off) = l;
    }
    char* sb = st + 3 * Cfg::PA;
#pragma unroll
    for (int p = 0; p < Cfg::PRB; ++p) {
      if (pc >= 0 && pc != Cfg::PRA + p) continue;
      const int cid = tid + Cfg::THREADS * p;
      const int r = cid >> 2;
      const int off = r * 64 + (((cid & 3) ^ x62_swz(r)) << 4);
      if constexpr (P3) {
        *reinterpret_cast<u32x4*>(sb + off) = rb3[q][p][0];
        *reinterpret_cast<u32x4*>(sb + Cfg::PB + off) = rb3[q][p][1];
        *reinterpret_cast<u32x4*>(sb + 2 * Cfg::PB + off) = rb3[q][p][2];
      } else {
        bf16x8 h, m, l;
        split3x8(rb[q][p][0], rb[q][p][1], h, m, l);
        *reinterpret_cast<bf16x8*>(sb + off) = h;
        *reinterpret_cast<bf16x8*>(sb + Cfg::PB + off) = m;
        *reinterpret_cast<bf16x8*>(sb + 2 * Cfg::PB + off) = l;
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (BN-backward epilogue: no bias -- the binding makes them exclusive -- so
  // no 16 bias registers beside its operand loads)
  float ssum[4][4], ssq[4][4], bia[BNB ? 1 : 4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      ssum[a][b] = ssq[a][b] = 0.f;
      if constexpr (!BNB) bia[a][b] = bias ? bias[n0 + wn * 64 + a * 16 + fq * 4 + b] : 0.f;
    }

  auto epilogue = [&](int64_t mt) __attribute__((always_inline)) {
    const int64_t mbase = mt * Cfg::BM;
    // BN-backward operands two fragments at a time (all four beside the
    // accumulators and the staged next slice spill at 256 VGPRs)
    constexpr int EH = BNB ? 1 : 4;
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      const int64_t m = mbase + wm * 64 + ms * 16 + fr;
      const bool live = m < M;
#pragma unroll
      for (int nh = 0; nh < 4; nh += EH) {
      f32x4 ehv[EH], ed2[EH];
      uint32_t ebits[EH];
      if constexpr (BNB) {
#pragma unroll
        for (int e = 0; e < EH; ++e) {
          ehv[e] = ed2[e] = f32x4{0.f, 0.f, 0.f, 0.f};
          ebits[e] = 0u;
        }
        if (live) {
          // compact dy2: output row m = (img, ph, pw) of the H x W grid adds dy2's row of
          // pixel (img, ph / 2, pw / 2) of the OH x OW grid when ph and pw are even, nothing
          // (-1) otherwise: two multiply-high divisions (the divisors' magic numbers come
          // with bb; M < 2^31, gemm.hip), written where the loads are so that nothing of
          // it stays live beside the accumulators (hoisted, the 8-wave tiles spilled more)
          int32_t d2row = -1;
          if constexpr (BNB && D2C) {
            const uint32_t mu = (uint32_t)m;
            const uint32_t img = (__umulhi(mu, bb.mg_hw) + mu) >> bb.sh_hw, rem = mu - img * (uint32_t)(bb.H * bb.W);
            const uint32_t ph = (__umulhi(rem, bb.mg_w) + rem) >> bb.sh_w, pw = rem - ph * (uint32_t)bb.W;
            if (((ph | pw) & 1u) == 0u) d2row = (int32_t)((img * (uint32_t)bb.OH + (ph >> 1)) * (uint32_t)bb.OW + (pw >> 1));
          }
#pragma unroll
          for (int e = 0; e < EH; ++e) {
            const int n = n0 + wn * 64 + (nh + e) * 16 + fq * 4;
            ehv[e] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.h) + m * ldc + n);
            if constexpr (D2C) {
              if (d2row >= 0)
                ed2[e] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.dy2) + (int64_t)d2row * ldc + n);
            } else {
              if (bb.dy2) ed2[e] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.dy2) + m * ldc + n);
            }
            ebits[e] = bb.mask ? (uint32_t)bb.mask[m * (Ntot >> 2) + (n >> 2)] : 0xfu;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < EH; ++e) {
        const int ns = nh + e;
        const int n = n0 + wn * 64 + ns * 16 + fq * 4;
        f32x4 v = acc[ms][ns];
        acc[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!BNB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bia[ns][r];
        }
        if constexpr (BNB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dz = (ebits[e] >> r) & 1u ? v[r] + ed2[e][r] : 0.f;
            v[r] = dz;
            ssum[ns][r] += dz;
            ssq[ns][r] = fmaf(dz, ehv[e][r], ssq[ns][r]);
          }
        } else {
          if (stats && live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              ssum[ns][r] += v[r];
              ssq[ns][r] = fmaf(v[r], v[r], ssq[ns][r]);
            }
          }
        }
        if (live) *reinterpret_cast<f32x4*>(C + m * ldc + n) = v;
      }
      }
    }
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, (NPF > 1 ? 1 : 0)>;
  // prologue: slice 0 into LDS stage 0, slices 1 .. NPF in flight
  issue_loads(I0{});
  split_write(0, I0{});
  if (T_ > 1) issue_loads(I1{});
  if (NPF > 1 && T_ > 2) issue_loads(I0{});
  __syncthreads();
  int ks = 0;
  int64_t mt = bx;
  // one K slice t (register set of slice t + 1: (t + 1) % NPF, compile-time through PAR = t % 2)
  auto slice = [&](int t, auto PAR) __attribute__((always_inline)) {
    constexpr int par = decltype(PAR)::value;
    using SN = std::integral_constant<int, (NPF > 1 ? (par ^ 1) : 0)>;   // set holding slice t + 1
    const int cur = par;
    const char* st = smem + cur * Cfg::STAGE;
    const char* pa = st;
    const char* pb = st + 3 * Cfg::PA;
    auto frag = [&](const char* plane, int row) __attribute__((always_inline)) -> bf16x8 {
      return *reinterpret_cast<const bf16x8*>(plane + row * 64 + ((fq ^ x62_swz(row)) << 4));
    };
    bf16x8 bh[4], bm[4], bl[4];
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) {
      const int row = wn * 64 + ns * 16 + fr;
      bh[ns] = frag(pb, row);
      bm[ns] = frag(pb + Cfg::PB, row);
      bl[ns] = frag(pb + 2 * Cfg::PB, row);
    }
    // The next slice's split pieces, plane writes and loads go between this
    // slice's MFMA groups (program order fixed by sched_barrier: a wave issues
    // in order, so VALU after a long MFMA run would wait for the matrix pipe
    // instead of filling the 8 of every 16 cycles an MFMA leaves free).
    constexpr int NPC = Cfg::PRA + Cfg::PRB;   // split pieces per thread per slice
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      const int row = wm * 64 + ms * 16 + fr;
      const bf16x8 ah = frag(pa, row), am = frag(pa + Cfg::PA, row), al = frag(pa + 2 * Cfg::PA, row);
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        f32x4 c = acc[ms][ns];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[ns], ah, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], al, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm[ns], am, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm[ns], ah, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], am, c, 0, 0, 0);
        acc[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], ah, c, 0, 0, 0);
        // step g = 4 ms + ns (16 steps): pieces on steps 1 .. NPC, the loads
        // on step NPC + 1 (all past the block's last slice too: the cursor
        // walks on over clamped, valid rows; the writes go to the stage nobody
        // reads again -- no branch, nothing for the scheduler to cluster around)
        const int gstep = 4 * ms + ns;
        if (gstep >= 1 && gstep <= NPC) split_write(cur ^ 1, SN{}, gstep - 1);
        if (gstep == NPC + 1) issue_loads(SN{});
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (++ks == nk) {
      ks = 0;
      epilogue(mt);
      mt += gridDim.x;
    }
    __syncthreads();
  };
  for (int t = 0; t < T_; t += 2) {
    slice(t, I0{});
    if (t + 1 < T_) slice(t + 1, std::integral_constant<int, 1>{});
  }

  if (stats) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          ssum[a][b] += __shfl_xor(ssum[a][b], off, 64);
          ssq[a][b] += __shfl_xor(ssq[a][b], off, 64);
        }
    float* red = reinterpret_cast<float*>(smem);   // [2][WM][BN]; every stage is consumed
    if (fr == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int col = wn * 64 + a * 16 + fq * 4 + b;
          red[wm * Cfg::BN + col] = ssum[a][b];
          red[(WM + wm) * Cfg::BN + col] = ssq[a][b];
        }
    }
    __syncthreads();
    for (int c = tid; c < Cfg::BN; c += Cfg::THREADS) {
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < WM; ++w2) {
        sa += red[w2 * Cfg::BN + c];
        sb += red[(WM + w2) * Cfg::BN + c];
      }
      stats[(int64_t)bx * Ntot + n0 + c] = sa;
      stats[stats_ld + (int64_t)bx * Ntot + n0 + c] = sb;
    }
  }
}

template <int WM, int WN, bool BNB, int NPF, bool GATHER, bool P3 = false, bool D2C = false>
int launch_nt_x62(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                  int K, int max_blocks, const float* bias, float* stats, int64_t stats_ld, int stats_rows,
                  const BnBwd& bb, const ConvGeo& geo, hipStream_t stream) {
  using Cfg = X62Cfg<WM, WN>;
  const int ntiles = N / Cfg::BN;
  const int64_t mtiles = (M + Cfg::BM - 1) / Cfg::BM;
  const int per_cu = (160 * 1024) / Cfg::LDS > 0 ? (160 * 1024) / Cfg::LDS : 1;
  int64_t gx = ((int64_t)256 * per_cu + ntiles - 1) / ntiles;
  if (max_blocks > 0) gx = max_blocks;
  if (gx < 1) gx = 1;
  if (gx > mtiles) gx = mtiles;
  if (stats && gx > stats_rows) gx = stats_rows;   // one partial row per block
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_x62_kernel<WM, WN, BNB, NPF, GATHER, P3, D2C>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL((gemm_nt_x62_kernel<WM, WN, BNB, NPF, GATHER, P3, D2C>), dim3((unsigned)gx, (unsigned)ntiles), dim3(Cfg::THREADS),
                     Cfg::LDS, stream, A, lda, B, ldb, C, ldc, M, K, bias, stats, stats_ld, bb, geo);
  return (int)gx;
}

// Reaches the instantiations that cfg::nt_x62_select can name (gemm_cfg.h: tiles, fallbacks).
// (two register sets in flight, NPF 2, measured slower everywhere: no longer instantiated)
template <bool GATHER>
int nt_x62_dispatch(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                    int N, int K, const cfg::NtWord& w, int max_blocks, const float* bias, float* stats,
                    int64_t stats_ld, int stats_rows, const BnBwd& bb, const ConvGeo& geo, hipStream_t stream) {
  const cfg::X62NtSel s = cfg::nt_x62_select(w, N, geo.b3 != nullptr, bb.h != nullptr);
// (D2C: the compact-dy2 epilogue, row GEMMs with the BN-backward epilogue only)
#define GK_X62L(WM_, WN_, BNB_, P3_, D2C_)                                                                   \
  launch_nt_x62<WM_, WN_, BNB_, 1, GATHER, P3_, D2C_>(A, lda, B, ldb, C, ldc, M, N, K, max_blocks, bias, stats, \
                                                      stats_ld, stats_rows, bb, geo, stream)
#define GK_X62N(WM_, WN_, P3_)                                             \
  do {                                                                     \
    if constexpr (!GATHER)                                                 \
      if (s.bnb && bb.OW > 0) return GK_X62L(WM_, WN_, true, P3_, true);   \
    return s.bnb ? GK_X62L(WM_, WN_, true, P3_, false) : GK_X62L(WM_, WN_, false, P3_, false); \
  } while (0)
#define GK_X62(WM_, WN_)               \
  case cfg::x62_key(WM_, WN_):         \
    if (s.p3) GK_X62N(WM_, WN_, true); \
    GK_X62N(WM_, WN_, false)
  switch (cfg::x62_key(s.wm, s.wn)) {
    GK_X62(2, 4);
    GK_X62(4, 2);
    GK_X62(1, 4);
    GK_X62(4, 1);
    GK_X62(1, 2);
    GK_X62(2, 1);
    GK_X62(2, 2);
  }
#undef GK_X62
#undef GK_X62N
#undef GK_X62L
  return cfg::kDoesNotFit;   // not reached: nt_x62_select names instantiated tiles only
}

}  // namespace
}  // namespace gk
