// Dump of the GEMM dispatch decisions (kernels/gemm_cfg.h) over a sweep of
// configuration words, call forms and shapes, one line of integers per call:
//   entry f32 bn lazy b3 geo cfg N K | status planes route elem x6 gather a b c d e f g
// entry: 0 gemm_nt, 1 conv_nt, 2 conv_nt_remap, 3 gemm_tn_acc, 4 conv_tn_acc
// geo:   0 one tap (C = K), 1 four taps (C = K / 4), 2 one tap, 32 images of 1024 x 1024
// route: 1 gemm_nt_kernel       a..g = WM WN MSB BNB LZ panel stages
//        2 gemm_tn_kernel       a..d = WN WK WS stages
//        3 gemm_tn_f32_kernel   a..d = WN WK LZ stages
//        4 gemm_nt_x62_kernel   a..d = WM WN P3 BNB
//        5 gemm_tn_x62_kernel   a..b = WN WK
// A refused call prints its status and zeros.  tests/test_gemm_cfg_cpu.py
// compares the output with tests/golden/gemm_dispatch.json.
#include <cstdio>
#include <cstdlib>

#include "gemm_cfg.h"

using namespace gk::cfg;

struct Call {
  int entry, f32, bn, lazy, b3, geo, cfg, N, K;
};

static void emit(const Call& c, int status, int planes, int route, int x6, int gather, int a, int b, int cc, int d,
                 int e, int f, int g) {
  const int elem = route == 0 ? 0 : (route == 2 || (route == 1 && !c.f32) ? 2 : 4);
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c.entry, c.f32, c.bn, c.lazy,
              c.b3, c.geo, c.cfg, c.N, c.K, status, planes, route, elem, x6, gather, a, b, cc, d, e, f, g);
}

static void nt_call(const Call& c) {
  const NtWord w = NtWord::decode(c.cfg);
  const bool remap = c.entry == 2;
  const bool gather = c.entry == 1 || (remap && c.geo == 1);
  const int C = c.geo == 1 ? c.K / 4 : c.K;
  const int64_t x_elems = c.geo == 2 ? (int64_t)32 * 1024 * 1024 * C : (int64_t)4 * 8 * 8 * C;
  const NtPlan p = nt_plan(w, c.f32, gather, c.lazy, c.b3, remap, w.planes > 1, c.K, C, x_elems);
  if (p.status < 0) return emit(c, p.status, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  // the split-K planes run the plain epilogue; the reduce pass has the fused one
  const bool bn = c.bn && p.planes == 1;
  if (p.unit == Unit::x62) {
    const X62NtSel s = nt_x62_select(w, c.N, c.b3, bn);
    return emit(c, 0, p.planes, 4, 1, gather, s.wm, s.wn, s.p3, s.bnb, 0, 0, 0);
  }
  const NtSel s = nt_select(w, c.N, c.f32, p.unit == Unit::x6, bn, c.lazy);
  emit(c, 0, p.planes, 1, p.unit == Unit::x6, gather, s.wm, s.wn, s.msb, s.bnb, s.lz, s.panel, s.stages);
}

static void tn_call(const Call& c) {
  const bool gather = c.entry == 4;
  if (!c.f32) {
    const TnSel s = tn_select(TnWord::decode(c.cfg), c.N, c.K);
    return emit(c, 0, 1, 2, 0, gather, s.wn, s.wk, s.ws, s.stages, 0, 0, 0);
  }
  const TnF32Word w = TnF32Word::decode(c.cfg);
  const TnPlan p = tn_plan(w, gather, c.lazy);
  if (p.status < 0) return emit(c, p.status, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  if (p.unit == Unit::x62) {
    const X62TnSel s = tn_x62_select(w, c.N, c.K);
    return emit(c, 0, 1, 5, 1, 0, s.wn, s.wk, 0, 0, 0, 0, 0);
  }
  const TnF32Sel s = tn_f32_select(w, c.N, c.K, c.lazy);
  emit(c, 0, 1, 3, p.unit == Unit::x6, gather, s.wn, s.wk, s.lz, s.stages, 0, 0, 0);
}

// ---- sweep ----------------------------------------------------------------
// every word of the file argv[1], as a bf16 and as an fp32 call
static const int kN[6] = {64, 128, 192, 256, 320, 512};
static const int kK[5] = {64, 128, 192, 256, 2048};

static void grid(Call c, void (*call)(const Call&)) {
  for (int n : kN)
    for (int k : kK) {
      c.N = n, c.K = k;
      call(c);
    }
}

int main(int argc, char** argv) {
  std::FILE* fp = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  if (!fp) return 2;
  int cfg;
  while (std::fscanf(fp, "%d", &cfg) == 1) {
    const int fam = (cfg / 100000) % 10;
    for (int f32 = 0; f32 < 2; ++f32) {
      const int nb3 = f32 && (fam == 2 || fam == 3) ? 2 : 1;
      for (int lazy = 0; lazy <= f32; ++lazy) {
        for (int bn = 0; bn < 2; ++bn)
          for (int b3 = 0; b3 < nb3; ++b3) {
            grid(Call{0, f32, bn, lazy, b3, 0, cfg, 0, 0}, nt_call);
            for (int geo = 0; geo < (nb3 == 2 ? 3 : 2); ++geo) grid(Call{1, f32, bn, lazy, b3, geo, cfg, 0, 0}, nt_call);
          }
        for (int geo = 0; geo < 2; ++geo) grid(Call{2, f32, 0, lazy, 0, geo, cfg, 0, 0}, nt_call);
        grid(Call{3, f32, 0, lazy, 0, 0, cfg, 0, 0}, tn_call);
        for (int geo = 0; geo < 2; ++geo) grid(Call{4, f32, 0, lazy, 0, geo, cfg, 0, 0}, tn_call);
      }
    }
  }
  std::fclose(fp);
  return 0;
}
