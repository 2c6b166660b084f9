// The GEMM configuration word: the one place that knows its format.
//
// Every gemm_nt / conv_nt / conv_dgrad_s2 / gemm_tn_acc / conv_tn_acc call is
// steered by one integer `cfg` (picked by the autotuner in ops/conv1x1.py,
// stored in tuning/gemm_choices.json).  Its decimal digits are fields; the
// gk:: entry points (gemm.hip) decode it once into one of the structs below
// and everything further down reads named fields.  This header also owns the
// tile selection (which template instantiation a decoded word means for a
// given N, K and call form, with every fallback rule and divisibility table)
// and the routing between the instantiation units, as pure functions: plain
// C++17, no HIP or torch includes, no heap use.
//
// NT word (forward / grad-input: gemm_nt, conv_nt, conv_nt_remap)
//   digit 1       tile; 0: auto by N.  Tiles BM x BN (waves):
//                   1 256x64 (4)  2 256x128 (8)  3 128x256 (8)  4 128x128 (4)
//                   5 256x256 (8, 128x64 per wave)  6 256x128 (4, 128x64)  7 128x256 (4, 128x64)
//                 fp32 runs 64x64 wave tiles (5-7 map to the 64x64 tile of the same
//                 block width) except the bf16x6 products, which keep 128x64.
//                 A tile above 7 or one whose width does not divide N becomes tile 1
//                 (B rows are not clamped).
//   digit 10      weight panel; 0: auto (resident when it fits), 1: resident in LDS, else streamed
//   digit 100     LDS stages; 1: two, 2: four, else three (a four-stage request falls back
//                 to three where the counts or the LDS do not fit: launch_nt_any)
//   digit 1000    fp32 only; 1: 32x64 wave tiles -- twice the waves of the 64x64 tiles for
//                 the small-M layers of small batches.  Its tiles:
//                   1 128x64 (4 waves)  2 64x128 (4)  3 64x64 (2)  4 32x256 (4)  5 128x128 (8)
//                   6 64x256 (8)  7 32x128 (2)
//                 checked against its own widths from the requested tile; ignored with a
//                 lazy operand
//   digit 10000   split-K planes S (> 1: S fp32 partial planes over K slices, then
//                 nt_splitk_reduce_kernel; fp32, no lazy operand, K divisible)
//   digit 100000  fp32 product family; 0: native v_mfma_f32_16x16x4_f32, 1: bf16x6 (X6,
//                 LDS-DMA staging), 2: bf16x6 with register staging ("x62"), 3: x62 with
//                 the B operand pre-split into bf16 planes by the caller (split3_rows).
//                 x62 tiles (WM, WN) of 64x64 wave tiles:
//                   1 (2,2) 128x128  2 (2,4) 128x256  3 (4,2) 256x128  4 (1,4) 64x256
//                   5 (4,1) 256x64  6 (1,2) 64x128  7 (2,1) 128x64
// TN bf16 word (grad-weight, bf16 operands)
//   tile = digit 1 + 10 * digit 100; 0: auto by N and K.  (WN, WK, WS), 64x64 per wave:
//     1 (1,1,4)  2 (2,1,2)  3 (1,2,2)  4 (2,2,1)  5 (4,1,1)  6 (1,4,1)  7 (2,2,2)  8 (1,1,2)
//     9 (4,2,1) 256x128  11 (2,4,1) 128x256  12 (4,4,1) 256x256 (16 waves): the large output
//     tiles halve the LDS-DMA / L2 traffic per MFMA of the compute-bound (long-K) grad-weights
//   digit 10      LDS stages; 2: three, else two
// TN fp32 word (grad-weight, fp32 operands)
//   digit 1       tile; 0: auto by N and K.  (WN, WK), 64x64 per wave:
//     1 (1,1)  2 (2,1)  3 (1,2)  4 (2,2)  5 (4,1)  6 (1,4)  7 (4,2)  8 (2,4)  9 (4,4)
//     (x62, family 2: tiles 1-8)
//   digit 10      LDS stages; 1: two, else three
//   digit 100000  product family as above (3 is refused: forward / grad-input only;
//                 2 takes the plain row form without a lazy operand)
#pragma once

#include <cstdint>

namespace gk {
namespace cfg {

// refusals of the gk:: entry points (any return value >= 0 is the grid size)
enum Status : int {
  kDoesNotFit = -1,    // lazy coefficient table too large for the tile's LDS, or a
                       // split-K request whose preconditions do not hold
  kRowGemmsOnly = -2,  // register-staged bf16x6 kernels asked for a form they do not take
  kCompactDy2 = -3,    // BN-backward epilogue with a compact dy2 (gk_kernels.h BnBwdArgs) on a
                       // call that is not one register-staged bf16x6 row GEMM
};

inline int family_of(int cfg) {
  const int f = (cfg / 100000) % 10;
  return f >= 1 && f <= 3 ? f : 0;
}

struct NtWord {
  int tile;      // requested tile, <= 0: auto
  int panel;     // -1: auto, 1: resident, 0: streamed
  int stages;    // 3, 2 or 4
  bool wave32;   // 32x64 wave-tile family (fp32)
  int planes;    // split-K planes, <= 1: none
  int family;    // fp32 product family 0-3
  static NtWord decode(int cfg) {
    const int p = (cfg / 10) % 10, s = (cfg / 100) % 10;
    return NtWord{cfg % 10,           p == 0 ? -1 : (p == 1 ? 1 : 0), s == 1 ? 2 : (s == 2 ? 4 : 3),
                  (cfg / 1000) % 10 == 1, (cfg / 10000) % 10,             family_of(cfg)};
  }
};

struct TnWord {
  int tile;     // <= 0: auto
  int stages;   // 2 or 3
  static TnWord decode(int cfg) { return TnWord{cfg % 10 + 10 * ((cfg / 100) % 10), (cfg / 10) % 10 == 2 ? 3 : 2}; }
};

struct TnF32Word {
  int tile;     // <= 0: auto
  int stages;   // 3 or 2
  int family;   // fp32 product family 0-3
  static TnF32Word decode(int cfg) {
    return TnF32Word{(cfg % 100000) % 10, (cfg / 10) % 10 != 1 ? 3 : 2, family_of(cfg)};
  }
};

// ---------------------------------------------------------------------------
// tile selection: the template arguments a decoded word stands for
// ---------------------------------------------------------------------------
struct NtSel {
  int wm, wn, msb;   // waves along M, N; 16-row MFMA subtiles per wave along M (2 / 4 / 8)
  bool bnb, lz;      // BN-backward epilogue, lazy A operand
  int panel, stages; // requests handed to launch_nt_any
};
constexpr int nt_key(int wm, int wn, int msb, bool bnb, bool lz) {
  return (((wm * 8 + wn) * 16 + msb) * 2 + (bnb ? 1 : 0)) * 2 + (lz ? 1 : 0);
}

// f32: fp32 operands (native or X6 unit); x6: the bf16x6 unit; bn: BN-backward
// epilogue present; lazy: lazy operand present (fp32 only)
inline NtSel nt_select(const NtWord& w, int N, bool f32, bool x6, bool bn, bool lazy) {
  static const int bn64[8] = {64, 64, 128, 256, 128, 256, 128, 256};
  int t = w.tile;
  if (t <= 0) t = N % 256 == 0 ? 3 : (N % 128 == 0 ? 2 : 1);
  if (t > 7 || N % bn64[t] != 0) t = 1;
  NtSel s{4, 1, 4, bn, f32 && lazy, w.panel, w.stages};
  if (f32 && w.wave32 && !lazy) {
    static const int bn32[8] = {64, 64, 128, 64, 256, 128, 256, 128};
    static const int wm32[8] = {4, 4, 2, 2, 1, 4, 2, 1}, wn32[8] = {1, 1, 2, 1, 4, 2, 4, 2};
    t = w.tile;
    if (t <= 0 || t > 7 || N % bn32[t] != 0) t = 1;
    s.wm = wm32[t], s.wn = wn32[t], s.msb = 2;
    return s;
  }
  if (bn || s.lz) {   // 64x64 wave tiles only
    static const int wm[8] = {4, 4, 4, 2, 2, 2, 2, 2}, wn[8] = {1, 1, 2, 4, 2, 4, 2, 4};
    s.wm = wm[t], s.wn = wn[t];
    return s;
  }
  // tiles 5-7: 128x64 wave tiles for bf16 and bf16x6 (fewer operand splits and LDS reads
  // per product); native fp32 runs the 64x64 wave tiles of the same block width
  static const int wm[8] = {4, 4, 4, 2, 2, 2, 2, 1}, wn[8] = {1, 1, 2, 4, 2, 4, 2, 4};
  s.wm = wm[t], s.wn = wn[t];
  if (t >= 5 && (!f32 || x6)) s.msb = 8;
  return s;
}

struct TnSel {
  int wn, wk, ws, stages;
};
constexpr int tn_key(int wn, int wk, int ws) { return (wn * 8 + wk) * 8 + ws; }

inline TnSel tn_select(const TnWord& w, int N, int K) {
  static const int bn[13] = {64, 64, 128, 64, 128, 256, 64, 128, 64, 256, 64, 128, 256};
  static const int bk[13] = {64, 64, 64, 128, 128, 64, 256, 128, 64, 128, 64, 256, 256};
  static const int wn[13] = {1, 1, 2, 1, 2, 4, 1, 2, 1, 4, 1, 2, 4}, wk[13] = {1, 1, 1, 2, 2, 1, 4, 2, 1, 2, 1, 4, 4};
  static const int ws[13] = {4, 4, 2, 2, 1, 1, 1, 2, 2, 1, 4, 1, 1};
  int t = w.tile;
  if (t <= 0) {
    const bool n2 = N % 128 == 0, k2 = K % 128 == 0;
    t = n2 && k2 ? 7 : (n2 ? 2 : (k2 ? 3 : 1));
  }
  if (t > 12 || t == 10 || N % bn[t] != 0 || K % bk[t] != 0) t = 1;   // tiles must divide N and K
  return TnSel{wn[t], wk[t], ws[t], w.stages};
}

struct TnF32Sel {
  int wn, wk;
  bool lz;
  int stages;   // request: three stages are kept where the tile's LDS fits (tn_f32_dispatch)
};
constexpr int tn_f32_key(int wn, int wk) { return wn * 8 + wk; }

inline TnF32Sel tn_f32_select(const TnF32Word& w, int N, int K, bool lazy) {
  static const int bn[10] = {64, 64, 128, 64, 128, 256, 64, 256, 128, 256};
  static const int bk[10] = {64, 64, 64, 128, 128, 64, 256, 128, 256, 256};
  int t = w.tile;
  if (t <= 0) t = (N % 128 == 0 && K % 128 == 0) ? 4 : (N % 128 == 0 ? 2 : (K % 128 == 0 ? 3 : 1));
  if (N % bn[t] != 0 || K % bk[t] != 0) t = 1;
  if (t == 9 && lazy) t = 8;   // the lazy 256x256 tile does not fit in LDS
  return TnF32Sel{bn[t] / 64, bk[t] / 64, lazy, w.stages};
}

struct X62NtSel {
  int wm, wn;
  bool p3, bnb;   // pre-split B operand, BN-backward epilogue
};
constexpr int x62_key(int a, int b) { return a * 8 + b; }

inline X62NtSel nt_x62_select(const NtWord& w, int N, bool b3, bool bn) {
  static const int bnw[8] = {128, 128, 256, 128, 256, 64, 128, 64};
  static const int wm[8] = {2, 2, 2, 4, 1, 4, 1, 2};
  int t = w.tile;
  if (t < 1 || t > 7 || N % bnw[t] != 0) t = N % 128 == 0 ? 1 : 7;
  if (N % bnw[t] != 0) t = 5;
  return X62NtSel{wm[t], bnw[t] / 64, b3, bn};
}

struct X62TnSel {
  int wn, wk;
};

inline X62TnSel tn_x62_select(const TnF32Word& w, int N, int K) {
  static const int bn[9] = {64, 64, 128, 64, 128, 256, 64, 256, 128};
  static const int bk[9] = {64, 64, 64, 128, 128, 64, 256, 128, 256};
  int t = w.tile;
  if (t < 1 || t > 8 || N % bn[t] != 0 || K % bk[t] != 0) t = 1;
  return X62TnSel{bn[t] / 64, bk[t] / 64};
}

// ---------------------------------------------------------------------------
// routing between the instantiation units (gemm.hip)
// ---------------------------------------------------------------------------
enum class Unit { b16, f32, x6, x62 };

// What an NT entry point does with a call: a refusal (status < 0), or `unit`
// runs it -- directly (planes == 1), or as `planes` split-K partial GEMMs over
// K / planes each (plain epilogue into the workspace) followed by the reduce.
struct NtPlan {
  int status;
  int planes;
  Unit unit;
};

// S split-K planes (S > 1) want K % (64 S) == 0 of a row GEMM and S dividing the
// (tap, channel) slices of 32 of an implicit one
inline bool splitk_divides(int S, bool gather, int K, int C) {
  return gather ? C % 32 == 0 && (K / 32) % S == 0 : K % (64 * S) == 0;
}

// remap: stride-2 grad-input output remap (conv_nt_remap; a split-K digit is
// ignored there); have_ws: the split-K workspace is there; K: the whole
// contraction length; C, x_elems: channels and images * H * W * C of the
// gathered operand (implicit GEMMs only).
inline NtPlan nt_plan(const NtWord& w, bool f32, bool gather, bool lazy, bool b3, bool remap, bool have_ws,
                      int K, int C, int64_t x_elems) {
  NtPlan p{0, 1, !f32 ? Unit::b16 : (w.family >= 2 ? Unit::x62 : (w.family == 1 ? Unit::x6 : Unit::f32))};
  if (!remap && w.planes > 1) {
    const int S = p.planes = w.planes;
    if (!f32 || lazy || !have_ws || !splitk_divides(S, gather, K, C)) p.status = kDoesNotFit;
  }
  if (p.status == 0 && p.unit == Unit::x62) {
    // bf16x6 with register staging: row GEMMs and stride / padding implicit GEMMs (C a
    // multiple of 32, 32-bit element offsets into x) without a lazy operand, split-K or
    // remap; family 3 wants the pre-split B operand, family 2 must not get one
    if (lazy || p.planes > 1 || remap || (w.family == 3) != b3) p.status = kRowGemmsOnly;
    else if (gather && (C % 32 != 0 || x_elems >= ((int64_t)1 << 31))) p.status = kRowGemmsOnly;
  }
  return p;
}

// The unit a fp32 grad-weight call runs on; status < 0: refused.
struct TnPlan {
  int status;
  Unit unit;
};

inline TnPlan tn_plan(const TnF32Word& w, bool gather, bool lazy) {
  TnPlan p{0, w.family == 2 ? Unit::x62 : (w.family == 1 ? Unit::x6 : Unit::f32)};
  // family 3 (pre-split B): forward / grad-input kernels only; family 2: the plain row form
  if (w.family == 3 || (w.family == 2 && (gather || lazy))) p.status = kRowGemmsOnly;
  return p;
}

}  // namespace cfg
}  // namespace gk
