// gemm_nt: 64*WM*WN threads, each wave owns a 64x64 output tile made of 4x4
//   v_mfma_f32_16x16x32_bf16 tiles.  Operands are K-contiguous, staged
//   global -> LDS with 16-byte global_load_lds (LDS-DMA) into 128-byte rows
//   (one 64-deep K slice) whose 16-byte chunks are XOR-swizzled by
//   (row >> 1) & 7, which makes every ds_read_b128 fragment read bank-conflict
//   free.  The MFMA is issued "swapped" (weight rows as the A operand, pixel
//   rows as B), so each lane ends with 4 consecutive output channels of one
//   pixel and writes them as one 8-byte store.  The grid is persistent over
//   M tiles and the two LDS stages are pipelined across tile boundaries, so
//   the next tile's loads are in flight during the current tile's MFMAs and
//   stores (the K = 64 layers have a single K step per tile).
#pragma once

#include "gemm_common.h"

namespace gk {
namespace {

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// --------------------------------------------------------------------------
// gemm_nt
// --------------------------------------------------------------------------
// BRES: the block's whole weight panel [BN x K] stays resident in LDS (it is
// the same for every M tile of the persistent loop); only A is streamed.
// NS: LDS stages; NS = 3 keeps two K slices in flight behind the one being
// multiplied.
// MSB: 16-row MFMA subtiles per wave along M (4: 64x64 wave tile, 8: 128x64 --
// fewer LDS reads per MFMA for the compute-bound shapes; bf16 only).
// T: element type, uint16_t (bf16 bits) or float.  A K slice is always one
// 128-byte LDS row per staged row -- 64 bf16 or 32 fp32 -- so staging,
// swizzle and fragment addressing are shared; a 16-byte fragment feeds one
// v_mfma_f32_16x16x32_bf16 (bf16) or four v_mfma_f32_16x16x4_f32 (fp32, exact
// fp32 products and sums: the reference's precision, no bf16 splitting).
template <typename T>
struct Elem {
  static constexpr bool F32 = sizeof(T) == 4;
  static constexpr int EPC = 16 / (int)sizeof(T);   // elements per 16-byte chunk
  static constexpr int KS = 8 * EPC;                // K elements per 128-byte slice row
  // 16-byte epilogue stores per 16-row subtile per wave (64 output columns)
  static constexpr int ST_PER_SUB = F32 ? 4 : 2;
};

template <int WM, int WN, bool BRES, int MSB = 4, typename T = uint16_t, bool LZ = false>
struct NtCfg {
  static constexpr int NW = WM * WN;
  static constexpr int THREADS = 64 * NW;
  static constexpr int WTM = 16 * MSB;            // wave tile rows
  static constexpr int BM = WTM * WM;
  static constexpr int BN = 64 * WN;
  static constexpr int ASTAGE = BM * 128;         // bytes: BM rows x one K slice
  static constexpr int NACOPY = LZ ? 2 : 1;       // lazy BN operand: dz and x tiles
  static constexpr int ASTAGES = NACOPY * ASTAGE;
  static constexpr int BSTAGE = BN * 128;
  static constexpr int STAGE = BRES ? ASTAGES : ASTAGES + BSTAGE;
  static constexpr int INSTS = STAGE / 1024;      // 1-KiB LDS-DMA instructions per stage
  static_assert(INSTS % NW == 0, "stage split");
  static constexpr int LPW = INSTS / NW;          // LDS-DMA instructions per wave per stage
  static_assert((BM / 8) % NW == 0, "A rows split evenly over the waves");
  static constexpr int LPWA = BRES ? LPW : NACOPY * (BM / 8) / NW;   // of which A-row instructions (j < LPWA)
  static constexpr int NST = Elem<T>::ST_PER_SUB * MSB;     // 16-byte epilogue stores per wave per tile
  static_assert(NST <= 63, "wait_vmcnt range (vmcnt is 6 bits)");
  static constexpr bool NS3_OK = LPW + 2 * NST <= 63;       // three stages: 1 stage + 2 tiles of stores in flight
  static constexpr bool NS4_OK = 2 * LPW + 3 * NST <= 63;   // four stages: 2 stages + 3 tiles of stores in flight
  // LDS: [lazy coefficient table][resident weight panel][stages]
  __host__ __device__ static int coef_bytes(int C) { return LZ ? ((C * 16 + 1023) / 1024) * 1024 : 0; }
  static int lds_bytes(int K, int ns, int C = 0) {
    return ns * STAGE + (BRES ? BN * K * (int)sizeof(T) : 0) + coef_bytes(C);
  }
};

template <int WM, int WN, bool BRES, int NS, bool GATHER, int MSB = 4, bool BNB = false, typename T = uint16_t,
          bool LZ = false, bool X6 = false>
__global__ void __launch_bounds__(64 * WM * WN) __attribute__((amdgpu_waves_per_eu(WM * WN >= 8 ? 1 : 2)))
gemm_nt_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
               T* __restrict__ C, int64_t ldc, int64_t M, int K, ConvGeo geo, float* __restrict__ stats,
               int64_t stats_ld, BnBwd bb, LazyA lz) {
  // stats != nullptr: per-block BatchNorm partials of the (dtype-rounded)
  // output, psum at stats[bx * N + n], psq at stats[stats_ld + ...]
  // (the [gy][C] layout bn_finalize_kernel reduces).  With bb.h (BN-backward
  // epilogue, MSB == 4 tiles only) the partials are sum(dz), sum(dz*h); the
  // finalize centres the second with the mean.
  using Cfg = NtCfg<WM, WN, BRES, MSB, T, LZ>;
  using E = Elem<T>;
  constexpr bool F32 = E::F32;
  static_assert(!LZ || F32, "lazy BN operand: fp32 kernels");
  static_assert(!X6 || F32, "bf16x6 products: fp32 operands");
  constexpr int EPC = E::EPC;
  constexpr int KS = E::KS;
  static_assert(!BNB || MSB == 4 || F32, "bf16 BN-backward epilogue: 64x64 wave tiles");
  static_assert(!F32 || MSB == 4 || MSB == 2 || (X6 && MSB == 8), "fp32: 64x64 or 32x64 wave tiles (bf16x6: 128x64)");
  static_assert(NS == 2 || (NS == 3 && Cfg::NS3_OK) || (NS == 4 && Cfg::NS4_OK), "wait_vmcnt range (vmcnt is 6 bits)");
  constexpr bool bnb = BNB;
  static_assert(NS >= 2 && NS <= 4, "stages");
  constexpr int LPW = Cfg::LPW;
  // split-K plane (ConvGeo::KZ): K is the per-plane depth; a gathered A starts
  // at the plane's first (tap, channel) slice instead of a column offset
  int kz_kh = 0, kz_kw = 0, kz_c0 = 0;
  if constexpr (!LZ) {
    if (gridDim.z > 1) {
      const int64_t z = blockIdx.z;
      if constexpr (GATHER) {
        const int per = geo.C / E::KS;   // K slices per tap
        const int s0 = (int)z * (K / E::KS);
        const int tap = s0 / per;
        kz_c0 = (s0 - tap * per) * E::KS;
        kz_kh = tap / geo.KW;
        kz_kw = tap - kz_kh * geo.KW;
      } else {
        A += z * K;
      }
      B += z * K;
      C += z * M * ldc;
    }
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int bx, by;   // logical block coordinates (XCD-aware order)
  xcd_remap2(bx, by);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: LDS-DMA M0 and fragment bases in SGPRs
  const int wm = wave / WN, wn = wave % WN;
  const int n0 = by * Cfg::BN;
  const int64_t mtiles = (M + Cfg::BM - 1) / Cfg::BM;
  const int nk = K / KS;
  // this block's work: M tiles bx, +gridDim.x, ...; each has nk K slices
  const int64_t my_tiles = bx < mtiles ? (mtiles - 1 - bx) / gridDim.x + 1 : 0;
  const int T_ = (int)(my_tiles * nk);
  const int Ntot = gridDim.y * Cfg::BN;
  if (T_ == 0) {
    if (stats)
      for (int c = threadIdx.x; c < Cfg::BN; c += Cfg::THREADS) {
        stats[(int64_t)bx * Ntot + n0 + c] = 0.f;
        stats[stats_ld + (int64_t)bx * Ntot + n0 + c] = 0.f;
      }
    return;
  }
  const int coefb = Cfg::coef_bytes(lz.C);
  char* panel = smem + coefb;
  char* stage_base = panel + (BRES ? Cfg::BN * K * (int)sizeof(T) : 0);
  if (LZ) {
    // lazy BN coefficients -> LDS (read back per fragment); drained before any
    // stage is issued, so the pipeline's vmcnt bookkeeping is untouched
    float4* ct = reinterpret_cast<float4*>(smem);
    const float4* cg = reinterpret_cast<const float4*>(lz.coef);
    for (int c = threadIdx.x; c < lz.C; c += Cfg::THREADS) ct[c] = cg[c];
    __syncthreads();
  }

  if (BRES) {  // weight panel: slice ks at panel + ks*BSTAGE, rows swizzled as the streamed tiles
    const int per = Cfg::BN / 8;
    for (int i = wave; i < nk * per; i += Cfg::NW) {
      const int ks = i / per, ri = i % per;
      const int r = ri * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz(r);
      glds16(B + (int64_t)(n0 + r) * ldb + ks * KS + c * EPC, (GK_LDS char*)panel + ks * Cfg::BSTAGE + ri * 1024);
    }
  }

  // ---- staging cursor: every per-lane address is set up once per M tile (A
  // rows) or once per kernel (B rows); a K step only adds the slice offset.
  // Instruction j of this wave fills staged rows i*8 .. i*8+7, i = wave + j*NW:
  // A rows while i*8 < BM, B rows after (streamed panel only).
  const T* ptr[LPW];          // A: row (or gathered pixel) base + chunk; B: row base + chunk
  // gather: bit kh of okh / bit kw of okw set when tap row kh / column kw of
  // this lane's output pixel lies inside the image (set once per M tile; a K
  // step tests two bits instead of recomputing and comparing the position)
  uint32_t okh[LPW], okw[LPW];
  const T* zrow[LPW];         // gather: this lane's chunk of the zero row (padding taps)
  // lazy operand: instructions i in [BM/8, 2 BM/8) stage the x tile; its
  // rows are the dz rows at a fixed element offset (same layout)
  const int64_t xoff = LZ ? static_cast<const T*>(lz.x) - A : 0;
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    const int i = wave + j * Cfg::NW;
    const int r = i * 8 + (lane >> 3);
    const int c = (lane & 7) ^ swz(r);
    const bool isx = LZ && i >= Cfg::BM / 8 && j < Cfg::LPWA;
    ptr[j] = j < Cfg::LPWA ? nullptr : B + (int64_t)(n0 + r - Cfg::NACOPY * Cfg::BM) * ldb + c * EPC;
    okh[j] = okw[j] = 0u;
    zrow[j] = !GATHER ? nullptr
              : LZ ? static_cast<const T*>(isx ? lz.padx : lz.padz) + c * EPC
                   : static_cast<const T*>(geo.zero) + c * EPC;
  }
  auto set_rows = [&](int64_t mt) {
    const int64_t m0 = mt * Cfg::BM;
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int i = wave + j * Cfg::NW;
      if (j < Cfg::LPWA) {
        const int ia = (LZ && i >= Cfg::BM / 8) ? i - Cfg::BM / 8 : i;   // row group within its A copy
        const int64_t xo = (LZ && i >= Cfg::BM / 8) ? xoff : 0;
        const int r = ia * 8 + (lane >> 3);
        const int c = (lane & 7) ^ swz(r);
        int64_t gr = m0 + r;
        gr = gr < M ? gr : M - 1;
        if (GATHER) {
          const uint32_t ohw = (uint32_t)(geo.OH * geo.OW);
          const uint32_t mu = (uint32_t)gr;
          const uint32_t n = mu / ohw, rem = mu - n * ohw;
          const uint32_t oh = rem / (uint32_t)geo.OW, ow = rem - oh * (uint32_t)geo.OW;
          const int ih0 = (int)oh * geo.S - geo.P;
          const int iw0 = (int)ow * geo.S - geo.P;
          uint32_t bh = 0u, bw = 0u;
#pragma unroll
          for (int q = 0; q < kMaxTaps; ++q) {   // host: KH, KW <= kMaxTaps
            bh |= (uint32_t)((unsigned)(ih0 + q) < (unsigned)geo.H) << q;
            bw |= (uint32_t)((unsigned)(iw0 + q) < (unsigned)geo.W) << q;
          }
          okh[j] = bh;
          okw[j] = bw;
          ptr[j] = A + xo + (((int64_t)n * geo.H + ih0) * geo.W + iw0) * geo.C + c * EPC;
        } else {
          ptr[j] = A + xo + gr * lda + c * EPC;
        }
      }
    }
  };
  int64_t s_mt = bx;    // tile of the next stage to issue
  int s_ks = 0;                 // its K slice
  int s_kh = kz_kh, s_kw = kz_kw, s_c0 = kz_c0;   // gather: tap and channel offset of that slice
  int s_t = 0;
  int s_buf = 0;                // LDS stage of the next issue (s_t % NS)
  set_rows(s_mt);
  // A stage is issued in three parts so the main loop can spread its LDS-DMA
  // instructions over the MFMA stream (stage_issue(j) between MFMA groups)
  // instead of issuing them back to back after the barrier, where their issue
  // cost (~60-180 cycles each among MFMAs, MI355X_MICROARCH.md LDS-DMA row)
  // left the matrix pipe idle at one wave per SIMD.
  GK_LDS char* st_base = nullptr;   // snapshot of the stage being issued
  int st_k0 = 0, st_kh = 0, st_kw = 0, st_c0 = 0;
  int64_t st_toff = 0;
  auto stage_prep = [&]() {
    st_base = (GK_LDS char*)stage_base + s_buf * Cfg::STAGE;
    st_k0 = s_ks * KS;
    st_toff = GATHER ? (int64_t)(s_kh * geo.W + s_kw) * geo.C + s_c0 : 0;   // wave-uniform
    st_kh = s_kh; st_kw = s_kw; st_c0 = s_c0;
  };
  auto stage_issue = [&](int j) {   // j: compile-time after unrolling
    const int i = wave + j * Cfg::NW;
    const T* src;
    if (j < Cfg::LPWA) {
      if (GATHER) {
        const bool ok = ((okh[j] >> st_kh) & (okw[j] >> st_kw) & 1u) != 0u;
        src = ok ? ptr[j] + st_toff : zrow[j] + (LZ ? st_c0 : 0);   // lazy: per-channel padding rows
      } else {
        src = ptr[j] + st_k0;
      }
    } else {
      src = ptr[j] + st_k0;
    }
    glds16(src, st_base + i * 1024);
  };
  auto stage_advance = [&]() {
    ++s_t;
    s_buf = s_buf + 1 == NS ? 0 : s_buf + 1;
    if (GATHER) {
      s_c0 += KS;
      if (s_c0 == geo.C) {
        s_c0 = 0;
        if (++s_kw == geo.KW) { s_kw = 0; ++s_kh; }
      }
    }
    if (++s_ks == nk) {
      s_ks = 0;
      s_kh = kz_kh; s_kw = kz_kw; s_c0 = kz_c0;
      s_mt += gridDim.x;
      if (s_t < T_) set_rows(s_mt);
    }
  };
  auto stage = [&]() {
    stage_prep();
#pragma unroll
    for (int j = 0; j < LPW; ++j) stage_issue(j);
    stage_advance();
  };

  f32x4 acc[MSB][4];
#pragma unroll
  for (int a = 0; a < MSB; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage();
  if (NS >= 3 && T_ > 1) stage();
  if (NS == 4 && T_ > 2) stage();
  const int fr = lane & 15, fq = lane >> 4;
  // stores issued by the last two steps (0 when none, or when a partial tile
  // drained its stores with vmcnt(0) right away)
  int st1 = 0, st2 = 0, st3 = 0;
  int ks = 0;
  int buf = 0;
  float ssum[4][4], ssq[4][4];   // BN partials: [ns][r] of this lane's column, summed over its rows
  float bia[4][4];               // bias of this lane's columns
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      ssum[a][b] = ssq[a][b] = 0.f;
      bia[a][b] = geo.bias ? geo.bias[n0 + wn * 64 + a * 16 + fq * 4 + b] : 0.f;
    }
  // bf16 BN-backward epilogue: in the store layout every lane owns 8 consecutive
  // channels per column pair pr (the same channels for every tile): offset
  // cofs within the pair's 32 columns
  const int cofs = (fq & 1) ? 16 + 4 * (fq - 1) : 4 * fq;
  // fp32 BN-backward epilogue operands (h, dy2, mask byte per 16-byte chunk)
  // of a 16-row subtile row ms.  The first PMS rows of a tile are loaded at
  // the start of its last K slice, so their latency hides under that slice's
  // MFMAs instead of stalling the epilogue; row ms + PMS is loaded into the
  // slot row ms frees while row ms is written.  (These loads are consumed
  // inside the same iteration, so the stage / store vmcnt accounting below is
  // unchanged.)
  // (32x64 wave tiles only: the 64x64 ones have no registers for it -- one
  // prefetched row already pushed them into 15-190 VGPRs of spills)
  constexpr bool PRE = F32 && BNB && MSB == 2;
  constexpr int PMS = PRE ? 2 : 1;
  f32x4 pre_h[PMS][4], pre_d[PMS][4];
  uint32_t pre_b[PMS][4];
  auto bn_row_load = [&](int64_t mbase_, int ms, f32x4* hh, f32x4* dd, uint32_t* bits) {
    const int64_t m = mbase_ + wm * Cfg::WTM + ms * 16 + fr;
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) {
      hh[ns] = dd[ns] = f32x4{0.f, 0.f, 0.f, 0.f};
      bits[ns] = 0u;
    }
    if (m < M) {
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        const int n = n0 + wn * 64 + ns * 16 + fq * 4;
        hh[ns] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.h) + m * ldc + n);
        if (bb.dy2) dd[ns] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.dy2) + m * ldc + n);
        bits[ns] = bb.mask ? (uint32_t)bb.mask[m * (Ntot >> 2) + (n >> 2)] : 0xfu;
      }
    }
  };
  int64_t mt = bx;
  for (int t = 0; t < T_; ++t) {
    // ops issued after stage(t), in order: NS=2: stores(t-1);
    // NS=3: stores(t-2), stage(t+1), stores(t-1).  Retire stage(t) only.
    // after stage(t): stores(t-NS+1..t-1) and the stages t+1 .. t+NS-2 issued since
    if (NS == 2) wait_vmcnt_fast<0>(st1);
    else if (NS == 3) wait_vmcnt_fast<LPW>(st2 + (t + 1 < T_ ? LPW : 0) + st1);
    else wait_vmcnt_fast<2 * LPW>(st3 + st2 + st1 + ((t + 1 < T_) + (t + 2 < T_)) * LPW);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const bool pf = s_t < T_;   // a stage to issue during this slice's MFMAs (wave-uniform)
    // fp32 spreads the next stage's LDS-DMA over the MFMA groups (16 fp32 MFMAs
    // per group hide each piece's issue cost); bf16 (4 MFMAs per group) issues
    // the whole stage right after the barrier -- measured on the ResNet-50
    // bs512 step: spreading cost bf16 ~1.4 ms (41.0 -> 42.4 ms); fp32 128.3 ms
    // with the previous tuning choices (128.1 before), 127.0 ms after a retune
    constexpr bool SPREAD = F32;
    if (pf) stage_prep();
    if constexpr (PRE) {
      if (ks == nk - 1) {
#pragma unroll
        for (int r = 0; r < PMS; ++r) bn_row_load(mt * Cfg::BM, r, pre_h[r], pre_d[r], pre_b[r]);
      }
    }
    if (!SPREAD && pf) {
#pragma unroll
      for (int q = 0; q < LPW; ++q) stage_issue(q);
    }
    const char* As = stage_base + buf * Cfg::STAGE;
    buf = buf + 1 == NS ? 0 : buf + 1;
    const char* Bs = BRES ? panel + ks * Cfg::BSTAGE : As + Cfg::ASTAGES;
    // lazy operand: channel of element 0 of this slice (K = taps x C, tap-major)
    const int cbase = LZ ? (ks * KS) % lz.C : 0;
    // MFMA groups per K slice: one per (half kk, 16-row subtile ms) -- fp32
    // 16 MFMAs (4 contraction slots x 4 subtiles), bf16 4; LDS-DMA piece q of
    // the next stage is issued after group (q * NG) / LPW
    constexpr int NG = 2 * MSB;
    auto issue_group = [&](int gi) {
      if constexpr (SPREAD) {
        if (pf) {
#pragma unroll
          for (int q = 0; q < LPW; ++q)
            if ((q * NG) / LPW == gi) stage_issue(q);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // Fragments: the 4 B fragments of a half are read one half ahead (both
    // halves' in flight at the slice start), the A fragment of subtile ms one
    // subtile ahead -- LDS latency hides under the previous group's MFMAs and
    // only ~40 (fp32) / ~24 (bf16) VGPRs of operands are live.
    // fp32: lane (fr, fq) holds K elements 16 kk + 4 fq + 0..3 of its row; MFMA
    // j contracts element j of every lane group (the same K permutation on
    // both operands, so the sum is the GEMM's).
    using Frag = typename std::conditional<F32, f32x4, bf16x8>::type;
    auto ldA = [&](int kk, int s) -> Frag {
      const int c = kk * 4 + fq;
      const int ra = wm * Cfg::WTM + s * 16 + fr;
      Frag v = *reinterpret_cast<const Frag*>(As + ra * 128 + ((c ^ swz(ra)) << 4));
      if constexpr (LZ) {
        // dx = k1 ((dz - k2) - (x - mu) k4) for channels cbase + 4c .. +3
        const float4* ct = reinterpret_cast<const float4*>(smem) + cbase + 4 * c;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(As + Cfg::ASTAGE + ra * 128 + ((c ^ swz(ra)) << 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 cf = ct[e];
          v[e] = cf.x * ((v[e] - cf.y) - (xv[e] - cf.z) * cf.w);
        }
      }
      return v;
    };
    // B fragments of both halves up front, except for the 128x64 bf16 wave
    // tiles (MSB 8: 128 accumulator VGPRs), which read each half's at its start
    constexpr int NBB = (F32 || MSB == 4) ? 2 : 1;
    Frag bv[NBB][4];
    auto ldB = [&](int kk, Frag* b) {
      const int c = kk * 4 + fq;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int rb = wn * 64 + s * 16 + fr;
        b[s] = *reinterpret_cast<const Frag*>(Bs + rb * 128 + ((c ^ swz(rb)) << 4));
      }
    };
    if constexpr (!F32) {
      // bf16: each half's A and B fragments read at its start, then its MFMAs
      // (the round-3 schedule; streaming A one subtile ahead measured slower here)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        Frag av[MSB], bh[4];
#pragma unroll
        for (int s2 = 0; s2 < MSB; ++s2) av[s2] = ldA(kk, s2);
        ldB(kk, bh);
#pragma unroll
        for (int ms = 0; ms < MSB; ++ms)
#pragma unroll
          for (int ns = 0; ns < 4; ++ns)
            acc[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], av[ms], acc[ms][ns], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < NBB; ++kk) ldB(kk, bv[kk]);
      if constexpr (X6) {
        // fp32-accurate products on the bf16 matrix cores: every fp32 operand
        // is split exactly into bf16 parts x = hi + mid + lo (split3x8) and the
        // six part products of order <= 2 -- all but mid*lo, lo*mid, lo*lo,
        // each < 2^-24 |a b| -- are accumulated in fp32.  Lane (fr, fq) holds
        // K elements 4 fq + 0..3 (half 0) and 16 + 4 fq + 0..3 (half 1) of its
        // row, the same permutation on both operands.  One K slice = one
        // 16x16x32 bf16 step: 6 x 16 cycles against 8 x 32 for the fp32 MFMA.
        bf16x8 bh[4], bm[4], bl[4];
        // Software-pipelined: the B splits of ns = 1..3 are interleaved with the
        // MFMAs of subtile row 0, the A split of subtile row ms + 1 with the
        // MFMAs of row ms (sched_group_barrier: 1 MFMA, then a few VALU) -- a
        // wave issues in order, so VALU placed after a run of MFMAs would wait
        // for the matrix pipe instead of filling its 16-cycle shadow.  (The first
        // form, all splits ahead of the MFMAs, measured within 1%: BASELINE.md.)
        split3x8(bv[0][0], bv[1][0], bh[0], bm[0], bl[0]);
        bf16x8 ah, am, al;
        {
          const Frag a0 = ldA(0, 0), a1 = ldA(1, 0);
          split3x8(a0, a1, ah, am, al);
        }
#pragma unroll
        for (int ms = 0; ms < MSB; ++ms) {
          Frag n0, n1;
          if (ms + 1 < MSB) {
            n0 = ldA(0, ms + 1);
            n1 = ldA(1, ms + 1);
          }
          bf16x8 nh, nm, nl;
#pragma unroll
          for (int ns = 0; ns < 4; ++ns) {
            if (ms == 0 && ns + 1 < 4) split3x8(bv[0][ns + 1], bv[1][ns + 1], bh[ns + 1], bm[ns + 1], bl[ns + 1]);
            if (ns == 1 && ms + 1 < MSB) split3x8(n0, n1, nh, nm, nl);
            f32x4 c = acc[ms][ns];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[ns], ah, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], al, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm[ns], am, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm[ns], ah, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], am, c, 0, 0, 0);
            acc[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[ns], ah, c, 0, 0, 0);
          }
          // schedule of this region: the next row's fragment reads first, then
          // the 24 MFMAs each followed by up to V VALU (ms 0: three B splits +
          // one A split, ~150 VALU; later rows: one A split, ~40)
          constexpr int V = 6;
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // DS reads
          if (ms == 0) {
#pragma unroll
            for (int q = 0; q < 24; ++q) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
              __builtin_amdgcn_sched_group_barrier(0x002, V, 0);   // VALU
            }
          } else {
#pragma unroll
            for (int q = 0; q < 24; ++q) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
            }
          }
          if (ms + 1 < MSB) {
            ah = nh;
            am = nm;
            al = nl;
          }
          issue_group(2 * ms);
          issue_group(2 * ms + 1);
        }
      } else {
      Frag an = ldA(0, 0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int sb = NBB == 2 ? kk : 0;
        if (NBB == 1 && kk == 1) ldB(1, bv[0]);
#pragma unroll
        for (int ms = 0; ms < MSB; ++ms) {
          const Frag a = an;
          if (ms + 1 < MSB) an = ldA(kk, ms + 1);
          else if (kk == 0) an = ldA(1, 0);
          if constexpr (F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int ns = 0; ns < 4; ++ns)
                acc[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[sb][ns][j], a[j], acc[ms][ns], 0, 0, 0);
          } else {
#pragma unroll
            for (int ns = 0; ns < 4; ++ns)
              acc[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv[sb][ns], a, acc[ms][ns], 0, 0, 0);
          }
          issue_group(kk * MSB + ms);
        }
      }
      }
    }
    if (pf) stage_advance();
    st3 = st2;
    st2 = st1;
    st1 = 0;
    if (++ks == nk) {
      ks = 0;
      // lane holds C[m = fr][n = 4*fq + r] of every 16x16 subtile.
      const int64_t mbase = mt * Cfg::BM;
      mt += gridDim.x;
      const bool full = mbase + Cfg::BM <= M;
      const bool odd = fq & 1;
#pragma unroll
      for (int ms = 0; ms < MSB; ++ms) {
        const int64_t m = mbase + wm * Cfg::WTM + ms * 16 + fr;
        const bool live = full || m < M;
        int64_t orow = m;     // output row (remapped for stride-2 grad-input classes)
        int zr = 0, zc = 0;   // RZ: sibling row / column inside the image
        if (geo.RH) {
          const uint32_t ohw = (uint32_t)(geo.OH * geo.OW);
          const uint32_t mu = (uint32_t)(m < M ? m : M - 1);
          const uint32_t ni = mu / ohw, rem = mu - ni * ohw;
          const uint32_t oh = rem / (uint32_t)geo.OW, ow = rem - oh * (uint32_t)geo.OW;
          orow = ((int64_t)ni * geo.RH + 2 * oh + geo.RA) * geo.RW + 2 * ow + geo.RB;
          zr = (int)(2 * oh + 1) < geo.RH;
          zc = (int)(2 * ow + 1) < geo.RW;
        }
        if constexpr (F32) {
          // fp32: lane owns 4 consecutive channels of every subtile -- one
          // 16-byte store per subtile, no shuffle.  BN-backward operands of the
          // row's four subtiles: prefetch slots (32x64 wave tiles) or loaded
          // here, all four before the first use.
          f32x4 ehv[4], ed2[4];
          uint32_t ebits[4];
          if constexpr (PRE) {
            const int slot = ms % PMS;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns) {
              ehv[ns] = pre_h[slot][ns];
              ed2[ns] = pre_d[slot][ns];
              ebits[ns] = pre_b[slot][ns];
            }
            if (ms + PMS < MSB) bn_row_load(mbase, ms + PMS, pre_h[slot], pre_d[slot], pre_b[slot]);
          } else if (bnb) {
#pragma unroll
            for (int ns = 0; ns < 4; ++ns) {
              ehv[ns] = ed2[ns] = f32x4{0.f, 0.f, 0.f, 0.f};
              ebits[ns] = 0u;
            }
            if (live) {
#pragma unroll
              for (int ns = 0; ns < 4; ++ns) {
                const int n = n0 + wn * 64 + ns * 16 + fq * 4;
                ehv[ns] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.h) + m * ldc + n);
                if (bb.dy2) ed2[ns] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(bb.dy2) + m * ldc + n);
                ebits[ns] = bb.mask ? (uint32_t)bb.mask[m * (Ntot >> 2) + (n >> 2)] : 0xfu;
              }
            }
          }
#pragma unroll
          for (int ns = 0; ns < 4; ++ns) {
            const int n = n0 + wn * 64 + ns * 16 + fq * 4;
            f32x4 v = acc[ms][ns];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += bia[ns][r];
            if (bnb) {
              // dz = mask ? dy + dy2 : 0; partials sum(dz), sum(dz * h)
              const f32x4 hv = ehv[ns], d2 = ed2[ns];
              const uint32_t bits = ebits[ns];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float dz = (bits >> r) & 1u ? v[r] + d2[r] : 0.f;
                v[r] = dz;
                ssum[ns][r] += dz;
                ssq[ns][r] = fmaf(dz, hv[r], ssq[ns][r]);
              }
            } else if (stats && live) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                ssum[ns][r] += v[r];
                ssq[ns][r] = fmaf(v[r], v[r], ssq[ns][r]);
              }
            }
            if (live) {
              *reinterpret_cast<f32x4*>(C + orow * ldc + n) = v;
              if (geo.RZ) {
                const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
                if (zc) *reinterpret_cast<f32x4*>(C + (orow + 1) * ldc + n) = z;
                if (zr) *reinterpret_cast<f32x4*>(C + (orow + geo.RW) * ldc + n) = z;
                if (zr && zc) *reinterpret_cast<f32x4*>(C + (orow + geo.RW + 1) * ldc + n) = z;
              }
            }
          }
        } else {
          // bf16: lanes fq and fq^1 swap halves of the subtile pair (2p, 2p+1) so
          // each lane owns 8 consecutive channels: one 16-byte store per lane per pair.
          uint4 eh[2], ed[2];   // BN-backward operands of this row: h, dy2 and the mask byte per pair
          uint32_t em[2];
          if (bnb) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
              const int n = n0 + wn * 64 + pr * 32 + cofs;
              eh[pr] = ed[pr] = make_uint4(0u, 0u, 0u, 0u);
              em[pr] = 0u;
              if (live) {
                eh[pr] = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(bb.h) + m * ldc + n);
                if (bb.dy2) ed[pr] = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(bb.dy2) + m * ldc + n);
                em[pr] = bb.mask ? (uint32_t)bb.mask[m * (Ntot >> 3) + (n >> 3)] : 0xffu;
              }
            }
          }
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const f32x4 va = acc[ms][2 * pr], vb = acc[ms][2 * pr + 1];
            const float* ba = bia[2 * pr];
            const float* bb2 = bia[2 * pr + 1];
            const uint32_t a0 = pack_bf16x2(va[0] + ba[0], va[1] + ba[1]), a1 = pack_bf16x2(va[2] + ba[2], va[3] + ba[3]);
            const uint32_t b0 = pack_bf16x2(vb[0] + bb2[0], vb[1] + bb2[1]), b1 = pack_bf16x2(vb[2] + bb2[2], vb[3] + bb2[3]);
            if (stats && !bnb && live) {   // statistics of the values as stored (bf16)
              const uint32_t pk[4] = {a0, a1, b0, b1};
#pragma unroll
              for (int h = 0; h < 4; ++h) {
                const float lo = __uint_as_float(pk[h] << 16), hi = __uint_as_float(pk[h] & 0xffff0000u);
                const int nsx = 2 * pr + (h >> 1), rr = (h & 1) * 2;
                ssum[nsx][rr] += lo;
                ssq[nsx][rr] = fmaf(lo, lo, ssq[nsx][rr]);
                ssum[nsx][rr + 1] += hi;
                ssq[nsx][rr + 1] = fmaf(hi, hi, ssq[nsx][rr + 1]);
              }
            }
            const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? a0 : b0), 16, 64);
            const uint32_t r1 = (uint32_t)__shfl_xor((int)(odd ? a1 : b1), 16, 64);
            uint4 v = odd ? make_uint4(r0, r1, b0, b1) : make_uint4(a0, a1, r0, r1);
            const int n = n0 + wn * 64 + pr * 32 + cofs;
            if (bnb) {
              const uint32_t dv[4] = {v.x, v.y, v.z, v.w};
              const uint4 e2 = ed[pr], eh4 = eh[pr];
              const uint32_t d2[4] = {e2.x, e2.y, e2.z, e2.w};
              const uint32_t hh[4] = {eh4.x, eh4.y, eh4.z, eh4.w};
              const uint32_t bits = em[pr];
              uint32_t o[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float lo = __uint_as_float(dv[i] << 16) + __uint_as_float(d2[i] << 16);
                float hi = __uint_as_float(dv[i] & 0xffff0000u) + __uint_as_float(d2[i] & 0xffff0000u);
                lo = (bits >> (2 * i)) & 1u ? lo : 0.f;
                hi = (bits >> (2 * i + 1)) & 1u ? hi : 0.f;
                o[i] = pack_bf16x2(lo, hi);
                const float hl = __uint_as_float(hh[i] << 16);
                const float hu = __uint_as_float(hh[i] & 0xffff0000u);
                const int a = 2 * pr + (i >> 1), b = (i & 1) * 2;
                ssum[a][b] += lo;
                ssq[a][b] = fmaf(lo, hl, ssq[a][b]);
                ssum[a][b + 1] += hi;
                ssq[a][b + 1] = fmaf(hi, hu, ssq[a][b + 1]);
              }
              v = make_uint4(o[0], o[1], o[2], o[3]);
            }
            if (live) {
              *reinterpret_cast<uint4*>(C + orow * ldc + n) = v;
              if (geo.RZ) {
                const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                if (zc) *reinterpret_cast<uint4*>(C + (orow + 1) * ldc + n) = z;
                if (zr) *reinterpret_cast<uint4*>(C + (orow + geo.RW) * ldc + n) = z;
                if (zr && zc) *reinterpret_cast<uint4*>(C + (orow + geo.RW + 1) * ldc + n) = z;
              }
            }
          }
        }
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) acc[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (full && !geo.RZ) st1 = Cfg::NST;
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // skipped / extra stores: keep the counts exact
    }
  }
  if (stats) {
    // sum over the 16 rows (lanes fr) of each lane group, then over the WM
    // waves sharing a column range, through LDS (every stage is consumed)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          ssum[a][b] += __shfl_xor(ssum[a][b], off, 64);
          ssq[a][b] += __shfl_xor(ssq[a][b], off, 64);
        }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);   // [2][WM][BN]
    if (fr == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          // forward and fp32: [subtile a][row b] of 4fq..; bf16 BN-backward:
          // store-layout channel cofs + 4 * (a & 1) + b of column pair a / 2
          const int col = (bnb && !F32) ? wn * 64 + (a >> 1) * 32 + cofs + (a & 1) * 4 + b
                                        : wn * 64 + a * 16 + fq * 4 + b;
          red[wm * Cfg::BN + col] = ssum[a][b];
          red[(WM + wm) * Cfg::BN + col] = ssq[a][b];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Cfg::BN; c += Cfg::THREADS) {
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

template <int WM, int WN, bool BRES, int NS, bool GATHER, int MSB = 4, bool BNB = false, typename T = uint16_t,
          bool LZ = false, bool X6 = false>
int launch_nt(const T* A, int64_t lda, const T* B, int64_t ldb, T* C, int64_t ldc, int64_t M,
              int N, int K, int max_blocks, const ConvGeo& geo, float* stats, int64_t stats_ld, int stats_rows,
              const BnBwd& bb, const LazyA& lz, hipStream_t stream) {
  using Cfg = NtCfg<WM, WN, BRES, MSB, T, LZ>;
  const int ntiles = N / Cfg::BN;
  const int64_t mtiles = (M + Cfg::BM - 1) / Cfg::BM;
  const int lds = Cfg::lds_bytes(K, NS, lz.C);
  const int per_cu = (160 * 1024) / lds > 0 ? (160 * 1024) / lds : 1;
  const int kz = (!LZ && geo.KZ > 1) ? geo.KZ : 1;
  int64_t gx = ((int64_t)256 * per_cu + ntiles * kz - 1) / (ntiles * kz);
  if (max_blocks > 0) gx = max_blocks;
  if (gx < 1) gx = 1;
  if (gx > mtiles) gx = mtiles;
  if (stats && gx > stats_rows) gx = stats_rows;   // one partial row per block
  dim3 grid((unsigned)gx, (unsigned)ntiles, (unsigned)kz);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_kernel<WM, WN, BRES, NS, GATHER, MSB, BNB, T, LZ, X6>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, BRES, NS, GATHER, MSB, BNB, T, LZ, X6>), grid, dim3(Cfg::THREADS), lds, stream,
                     A, lda, B, ldb, C, ldc, M, K, geo, stats, stats_ld, bb, lz);
  return (int)gx;
}

template <int WM, int WN, bool GATHER, int MSB = 4, bool BNB = false, typename T = uint16_t, bool LZ = false,
          bool X6 = false>
int launch_nt_any(const T* A, int64_t lda, const T* B, int64_t ldb, T* C, int64_t ldc,
                  int64_t M, int N, int K, int max_blocks, int bres, int ns, const ConvGeo& geo, float* stats,
                  int64_t stats_ld, int stats_rows, const BnBwd& bb, const LazyA& lz, hipStream_t stream) {
  using CR = NtCfg<WM, WN, true, MSB, T, LZ>;
  using CS = NtCfg<WM, WN, false, MSB, T, LZ>;
  const int cc = lz.C;
  // keep the weight panel resident when it fits next to the two A stages
  if (bres < 0) bres = (64 * WN) * K * (int)sizeof(T) <= 64 * 1024;
  if (bres && CR::lds_bytes(K, 2, cc) > 160 * 1024) bres = 0;
  constexpr int L = 160 * 1024;
#define GK_NT(BR, S) \
  launch_nt<WM, WN, BR, S, GATHER, MSB, BNB, T, LZ, X6>(A, lda, B, ldb, C, ldc, M, N, K, max_blocks, geo, stats, stats_ld, stats_rows, bb, lz, stream)
  if constexpr (CR::NS4_OK)
    if (ns == 4 && bres && CR::lds_bytes(K, 4, cc) <= L) return GK_NT(true, 4);
  if constexpr (CS::NS4_OK)
    if (ns == 4 && !bres && CS::lds_bytes(K, 4, cc) <= L) return GK_NT(false, 4);
  if (bres) {
    if constexpr (CR::NS3_OK)
      if (ns != 2 && CR::lds_bytes(K, 3, cc) <= L) return GK_NT(true, 3);
    return GK_NT(true, 2);
  }
  if constexpr (CS::NS3_OK)
    if (ns != 2 && CS::lds_bytes(K, 3, cc) <= L) return GK_NT(false, 3);
  if (CS::lds_bytes(K, 2, cc) > L) return cfg::kDoesNotFit;   // lazy coefficient table too large
  return GK_NT(false, 2);
#undef GK_NT
}

// Reaches the instantiations that cfg::nt_select can name; the tile tables and the
// fallback rules are in gemm_cfg.h.
template <bool GATHER, typename T, bool X6 = false>
int nt_dispatch(GK_NT_UNIT_ARGS) {
  auto a = static_cast<const T*>(A);
  auto b = static_cast<const T*>(B);
  auto c = static_cast<T*>(C);
  const cfg::NtSel s = cfg::nt_select(w, N, sizeof(T) == 4, X6, bb.h != nullptr, lza != nullptr);
  const LazyA lz = lza ? LazyA{lza->x, lza->coef, lza->padz, lza->padx, lza->C} : LazyA{};
#define GK_NTA(WM_, WN_, MSB_, BNB_, LZ_)                                                                           \
  case cfg::nt_key(WM_, WN_, MSB_, BNB_, LZ_):                                                                      \
    return launch_nt_any<WM_, WN_, GATHER, MSB_, BNB_, T, LZ_, X6>(a, lda, b, ldb, c, ldc, M, N, K, max_blocks, s.panel, \
                                                                   s.stages, geo, stats, stats_ld, stats_rows, bb, lz, stream)
  // the four 64x64-wave-tile blocks and the seven 32x64 ones (case order = instantiation order)
#define GK_NT64(BNB_, LZ_)          \
  GK_NTA(4, 2, 4, BNB_, LZ_);       \
  GK_NTA(2, 4, 4, BNB_, LZ_);       \
  GK_NTA(2, 2, 4, BNB_, LZ_);       \
  GK_NTA(4, 1, 4, BNB_, LZ_)
#define GK_NT32(BNB_)               \
  GK_NTA(2, 2, 2, BNB_, false);     \
  GK_NTA(2, 1, 2, BNB_, false);     \
  GK_NTA(1, 4, 2, BNB_, false);     \
  GK_NTA(4, 2, 2, BNB_, false);     \
  GK_NTA(2, 4, 2, BNB_, false);     \
  GK_NTA(1, 2, 2, BNB_, false);     \
  GK_NTA(4, 1, 2, BNB_, false)
  const int key = cfg::nt_key(s.wm, s.wn, s.msb, s.bnb, s.lz);
  if constexpr (sizeof(T) == 4) {
    switch (key) {
      GK_NT64(true, true);   // lazy BN-backward A operand
      GK_NT64(false, true);
      GK_NT32(true);
      GK_NT32(false);
      GK_NT64(true, false);
    }
    if constexpr (X6) {   // bf16x6: 128x64 wave tiles
      switch (key) {
        GK_NTA(2, 4, 8, false, false);
        GK_NTA(2, 2, 8, false, false);
        GK_NTA(1, 4, 8, false, false);
      }
    }
    switch (key) {
      GK_NTA(4, 2, 4, false, false);
      GK_NTA(2, 4, 4, false, false);
      GK_NTA(1, 4, 4, false, false);
      GK_NTA(2, 2, 4, false, false);
      GK_NTA(4, 1, 4, false, false);
    }
  } else {
    switch (key) {
      GK_NT64(true, false);
      GK_NTA(4, 2, 4, false, false);
      GK_NTA(2, 4, 4, false, false);
      GK_NTA(2, 2, 4, false, false);
      GK_NTA(2, 4, 8, false, false);
      GK_NTA(2, 2, 8, false, false);
      GK_NTA(1, 4, 8, false, false);
      GK_NTA(4, 1, 4, false, false);
    }
  }
#undef GK_NT32
#undef GK_NT64
#undef GK_NTA
  return cfg::kDoesNotFit;   // not reached: nt_select names instantiated tiles only
}

}  // namespace
}  // namespace gk
