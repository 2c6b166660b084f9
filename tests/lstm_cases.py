"""Shared cases of the LSTM kernel tests (csrc/kernels/lstm.hip): the three split-K step GEMMs (bf16, fp32,
bf16x6) and the templated forward / backward cell kernels.  tests/test_lstm_edges_cpu.py runs them through
torch mirrors (the step GEMMs, slice by slice and K batch by K batch in the kernel's precision) and the
PyTorch fallback of ``ops.lstm`` (``_cell_fwd_ref`` / ``_cell_bwd_ref``); tests/test_lstm_edges_gpu.py runs
the same runners on the raw ``torch.ops.gksgd`` ops.  Every runner takes the device; every reference is fp64
PyTorch on the CPU, on the inputs as stored, written from the formulas in the header of lstm.hip without
autograd, computed once per case and shared (``functools.lru_cache``).  The backward takes ``gates``, ``c``
and ``c_prev`` as stored fp32 tensors -- the fp64 forward rounded once -- so the kernel and the reference
differentiate the same numbers.

Tolerance rules
---------------
The rules (and ``Tally``, ``FACTOR``, ``BF16_ULP``, ``FP32_SUM``) are those of tests/bert_row_cases.py; no
rule looks at the output under test to size itself, and there are no undecided elements.

bit-equal   step GEMMs on integer operands in [-8, 8] (exact in bf16; on bf16x6 they sit entirely in the hi
            plane, mid = lo = 0).  With K <= 1536 every partial sum satisfies |sum| <= 64 * 1536 = 98304 <
            2^24, so every fp32 accumulation in any order is exact and every slice P[s] must equal the fp64
            product of its own K range bit for bit: any permutation, dropped or doubled K step, wrong slice
            offset or unwritten element (P is pre-filled with NaN) shows.  The strided scenario holds the
            strided call against the dense call of the same kernel bit for bit as well.

1. bf16-stored h / dG of the cell kernels: elementwise ``|ours - ref| <= 2^-8 |ref| + E``, E the fp32 bound
   of rule 3 for that tensor.

2. fp32 sum of ``n`` exact fp32 terms in any order: elementwise ``|ours - ref| <= n 2^-23 sum|terms|``, per
   slice.  bf16 step GEMM: n = ks (the products of two bf16 values are exact in fp32).  fp32 step GEMM:
   n = ks + 1 (one more for the rounding of every product).  bf16x6: the six part products of order <= 2 are
   exact in fp32 as well, so n = 6 ks + 1 over sum (|a_hi| + |a_mid| + |a_lo|)(|b_hi| + |b_mid| + |b_lo|);
   the + 1 covers the three dropped products (each < 2^-24 |a b|).  On bf16x6 this elementwise bound is loose
   (it only keeps a single wrong element from hiding in a norm); its accuracy is held by rule 3.

3. the yardstick.  bf16x6 step GEMM: the relative Frobenius error of every slice against fp64 is held against
   the same error of PyTorch's fp32 CPU ``A @ B.t()`` on the same operands, times ``FACTOR`` (= 2: room for
   six times as many fp32 additions in another order).  Six exact part products are 0.02 - 0.04 x the CPU
   fp32 error at these depths; dropping one second-order product (mid * mid, hi * lo) is 8 - 19 x.
   Cell kernels: the fp32 tensors (c, gates, dc_prev on both storage types; h, dG with fp32 storage) are
   held to ``FACTOR`` x the max-abs error against fp64 of the fp32 PyTorch CPU composition
   (``torch.sigmoid`` / ``torch.tanh``, the same order of additions as the kernel), per tensor.  The
   yardstick is taken from the POOL case (64, 320) of the same input distribution, path and slice count and
   applied to the small shapes: a one-element case has a yardstick of pure luck (c: 1.3e-8 at (1, 1) against
   3.7e-7 at the pool shape).  The saturation case (50000 elements, every combination of the saturating
   values) is the pool of its own input distribution: its yardstick is the composition's error on itself.

Refusals.  The step-GEMM refusals run on both sides (the torch mirrors repeat the bindings' checks).  The
refusals of ``lstm_cell_fwd`` / ``lstm_cell_bwd`` run on the GPU only: off the GPU the cells are plain
PyTorch functions without a binding whose checks could be mirrored.

Every check prints ``TOL | family | case | tensor | rule | err | bound | ratio``;
profiles/lstm_kernels_tolerances.txt is the worst line per family and tensor of the GPU run.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import torch

from bert_row_cases import BF16, BF16_ULP, F32, F64, FACTOR, FP32_SUM, Tally, is_gpu  # noqa: F401

NAN = float("nan")
SENTINEL = 7.0
GUARD = 4096          # sentinel floats on each side of P in the strided scenario


def cdname(cd):
    return "bf16" if cd == BF16 else "fp32"


def pad64(n):
    return (n + 63) // 64 * 64


def _c64(t):
    return t.detach().to("cpu", F64)


def at1(t, device, junk=NAN):
    """``t`` on ``device`` as the [1] slice of a [2, ...] tensor: contiguous, storage offset t.numel() (odd
    for an odd element count, so nothing may assume more than element alignment)."""
    buf = torch.full((2,) + tuple(t.shape), junk, dtype=t.dtype, device=device)
    buf[1].copy_(t)
    return buf[1]


def out1(shape, dt, device):
    """An output as the middle slice of a sentinel-filled [3, ...] buffer: (view, buffer)."""
    buf = torch.full((3,) + tuple(shape), SENTINEL, dtype=dt, device=device)
    return buf[1], buf


def yard_abs(t, case, name, ours, ref, y):
    """Rule 3 with a given yardstick ``y`` (a max-abs error): max|ours - ref| <= FACTOR y."""
    ours, ref = _c64(ours), _c64(ref)
    assert ours.shape == ref.shape, (case, name, ours.shape, ref.shape)
    d = (ours - ref).abs()
    err = NAN if torch.isnan(d).any() else float(d.max())
    t._rec(case, name, "yardstick", err, y, err / y if y > 0 else (0.0 if err == 0 else math.inf), FACTOR)


# --------------------------------------------------------------------------- R. the split-K step GEMMs

KINDS = ("bf16", "fp32", "x6")
COMPILED = {"bf16": (2, 4, 8), "fp32": (4, 8), "x6": (2,)}     # the D of every instantiated kernel
KSTEP = {"bf16": 32, "fp32": 16, "x6": 32}                     # K depth of one of the D steps of a batch


def rec_variant(kind, ks):
    """(D, trips) of the kernel that ``lstm_rec_gemm`` / ``lstm_rec_gemm_f32`` / ``lstm_rec_gemm_x6`` launch for
    a slice depth ks = K / S: the ``ks %`` ladders of lstm.hip written out."""
    assert ks > 0 and ks % 64 == 0, ks          # the bindings demand K % (64 S) == 0
    if kind == "bf16":
        D = 8 if ks % 256 == 0 else (4 if ks % 128 == 0 else 2)
    elif kind == "fp32":
        D = 8 if ks % 128 == 0 else 4
    else:
        D = 2
    assert ks % (KSTEP[kind] * D) == 0
    return D, ks // (KSTEP[kind] * D)


# (M, N, ks, S): K = S ks <= 1536
GEMM_CASES = {
    "bf16": [(1, 64, 64, 1), (16, 64, 192, 2), (17, 192, 128, 3), (33, 64, 384, 1), (65, 64, 256, 2),
             (96, 64, 512, 3), (97, 192, 64, 3), (128, 64, 192, 1), (129, 64, 128, 2), (257, 64, 384, 3),
             (33, 192, 512, 1), (129, 64, 256, 1)],
    "fp32": [(1, 64, 64, 1), (16, 64, 192, 2), (17, 192, 128, 3), (33, 64, 256, 1), (65, 64, 64, 3),
             (96, 64, 192, 1), (97, 192, 128, 2), (128, 64, 256, 3), (129, 64, 64, 2), (257, 64, 192, 3),
             (33, 192, 256, 2), (129, 64, 128, 1)],
    "x6": [(1, 64, 64, 1), (16, 64, 192, 2), (17, 192, 64, 3), (33, 64, 192, 1), (65, 64, 64, 2),
           (96, 64, 192, 3), (97, 192, 64, 1), (128, 64, 192, 2), (129, 64, 64, 3), (257, 64, 192, 1),
           (33, 192, 192, 3), (257, 64, 64, 2)],
}
GEMM_M = (1, 16, 17, 33, 97, 128, 129, 257)


def _split3(w):
    from gaussiank_sgd_amd.ops.lstm import split3
    return split3(w)


@functools.lru_cache(maxsize=None)
def gemm_case(kind, M, N, ks, S, mode):
    """Operands (as stored), the fp64 product of every slice, sum|terms| of rule 2 and, for bf16x6, the
    relative Frobenius error of PyTorch's fp32 CPU product of every slice."""
    K = S * ks
    gen = torch.Generator().manual_seed(M * 7919 + N * 31 + K + S + KINDS.index(kind) * 100003)
    if mode == "exact":
        A = torch.randint(-8, 9, (M, K), generator=gen).float()
        B = torch.randint(-8, 9, (N, K), generator=gen).float()
    else:
        A = torch.randn(M, K, generator=gen)
        B = torch.randn(N, K, generator=gen) * K ** -0.5
    if kind == "bf16":
        A, B = A.to(BF16), B.to(BF16)
    c = SimpleNamespace(kind=kind, M=M, N=N, ks=ks, S=S, K=K, A=A, B=B, B3=None)
    a64, b64 = A.double(), B.double()
    aabs, babs = a64.abs(), b64.abs()
    if kind == "x6":
        c.B3 = _split3(B)
        A3 = _split3(A).double()
        assert torch.equal(c.B3.double().sum(0), b64) and torch.equal(A3.sum(0), a64)     # the split is exact
        if mode == "exact":
            assert not c.B3[1:].float().any() and not A3[1:].any()                         # all in the hi plane
        aabs, babs = A3.abs().sum(0), c.B3.double().abs().sum(0)
    sl = [slice(s * ks, (s + 1) * ks) for s in range(S)]
    c.ref = torch.stack([a64[:, k] @ b64[:, k].t() for k in sl])
    c.sumabs = torch.stack([aabs[:, k] @ babs[:, k].t() for k in sl])
    if mode == "exact":
        assert float(c.sumabs.max()) < 2 ** 24
    if kind == "x6":
        c.yard = [float((torch.mm(A[:, k], B[:, k].t()).double() - r).norm() / r.norm()) for k, r in zip(sl, c.ref)]
    return c


def assert_case_table():
    """From the dispatch mirror: the tables reach every compiled (kernel, D) with one trip and with >= 2 trips,
    M mod 128 in each quarter of a tile, M > 128 and M > 256, S in {1, 2, 3}, both N -- and the cell tables
    every geometry the cell kernels can meet."""
    for kind in KINDS:
        rows = GEMM_CASES[kind]
        hit = {(rec_variant(kind, ks)[0], min(rec_variant(kind, ks)[1], 2)) for _, _, ks, _ in rows}
        assert hit == {(D, n) for D in COMPILED[kind] for n in (1, 2)}, (kind, hit)
        last = [((M - 1) % 128) + 1 for M, _, _, _ in rows]        # rows of the last 128-row tile
        for lo, hi in ((0, 32), (32, 64), (64, 96), (96, 127)):    # 1 .. 4 waves stay, the last one partial
            assert any(lo < m <= hi for m in last), (kind, lo, hi)
        assert any(m == 128 for m in last)
        ms = {M for M, _, _, _ in rows}
        assert set(GEMM_M) <= ms and any(128 < M <= 256 for M in ms) and any(M > 256 for M in ms), (kind, ms)
        assert {S for _, _, _, S in rows} == {1, 2, 3} and {N for _, N, _, _ in rows} == {64, 192}
        assert all(S * ks <= 1536 for _, _, ks, S in rows)
    rows = CELL_CASES + [POOL_CASE]
    n = [B * H for B, H, _, _ in rows]
    assert any(v < 256 for v in n) and any(v == 256 for v in n), "one partial block, exactly one block"
    assert any(v > 256 and v % 256 for v in n), "several blocks with a tail"
    assert any(v > 256 and v % 256 == 0 for v in n), "several whole blocks"
    assert any(pad64(H) == H for _, H, _, _ in rows) and any(pad64(H) - H == 63 for _, H, _, _ in rows)
    assert sum(1 for _, _, extra, _ in rows if extra) == 1, "Hp > pad64(H) once"
    assert {S for _, _, _, S in rows} == {1, 3}
    assert any(v % 2 for v in n) and any(v % 2 == 0 for v in n), "odd and even storage offsets"
    assert {(B, H) for B, H, _, _ in CELL_CASES} == {(1, 1), (1, 64), (1, 65), (3, 40), (1, 256), (1, 257), (5, 63),
                                                     (129, 3)}


# ---- the torch mirror: the bindings' checks, then slice by slice, K batch by K batch

def _refuse(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _check_p(P, numel):
    _refuse(P.dtype == F32 and P.is_contiguous() and P.numel() == numel, "P must be a contiguous fp32 tensor of "
            "%d elements" % numel)


def mirror_rec_gemm(A, Bm, P, S):
    """bindings.cpp lstm_rec_gemm off the GPU: the same refusals, then rec_gemm_kernel / rec_gemm_f32_kernel."""
    _refuse(A.dim() == 2 and Bm.dim() == 2 and A.size(1) == Bm.size(1), "A [M, K] and B [N, K] expected")
    M, K, N = A.size(0), A.size(1), Bm.size(0)
    _refuse(S >= 1 and K % (64 * S) == 0 and N % 64 == 0, "K % (64 S) and N % 64 must be 0")
    dt = F32 if A.dtype == F32 else BF16
    al = 4 if dt == F32 else 8
    _refuse(all(x.dtype == dt and x.stride(1) == 1 and x.stride(0) % al == 0 for x in (A, Bm)),
            "bf16 or fp32 operands (both alike) with unit column stride and 16-byte aligned rows")
    _refuse(A.data_ptr() % 16 == 0 and Bm.data_ptr() % 16 == 0, "16-byte aligned operands")
    _check_p(P, S * M * N)
    kind = "fp32" if dt == F32 else "bf16"
    ks = K // S
    D, trips = rec_variant(kind, ks)
    step = KSTEP[kind] * D
    out = P.view(S, M, N)
    for s in range(S):
        acc = torch.zeros(M, N)
        for i in range(trips):
            k = slice(s * ks + i * step, s * ks + (i + 1) * step)
            acc = acc + torch.mm(A[:, k].float(), Bm[:, k].float().t())
        out[s].copy_(acc)


def mirror_rec_gemm_x6(A, B3, P, S):
    """bindings.cpp lstm_rec_gemm_x6 off the GPU: A split into three bf16 parts, six part products per K batch
    accumulated in fp32, smallest first (the order of rec_gemm_x6_kernel)."""
    _refuse(A.dim() == 2 and B3.dim() == 3 and B3.size(0) == 3 and A.size(1) == B3.size(2),
            "A [M, K] fp32 and B3 [3, N, K] bf16 expected")
    M, K, N = A.size(0), A.size(1), B3.size(1)
    _refuse(S >= 1 and K % (64 * S) == 0 and N % 64 == 0, "K % (64 S) and N % 64 must be 0")
    _refuse(A.dtype == F32 and A.stride(1) == 1 and A.stride(0) % 4 == 0 and B3.dtype == BF16 and
            B3.stride(2) == 1 and B3.stride(1) % 8 == 0 and B3.stride(0) % 8 == 0,
            "fp32 A / bf16 B3 operands with unit column stride and 16-byte aligned rows")
    _refuse(A.data_ptr() % 16 == 0 and B3.data_ptr() % 16 == 0, "16-byte aligned operands")
    _check_p(P, S * M * N)
    ks = K // S
    D, trips = rec_variant("x6", ks)
    step = KSTEP["x6"] * D
    out = P.view(S, M, N)
    for s in range(S):
        acc = torch.zeros(M, N)
        for i in range(trips):
            k = slice(s * ks + i * step, s * ks + (i + 1) * step)
            ah, am, al = (p.float() for p in _split3(A[:, k].contiguous()))
            bh, bm, bl = (p.float().t() for p in B3[:, :, k])
            for a, b in ((al, bh), (ah, bl), (am, bm), (ah, bm), (am, bh), (ah, bh)):
                acc = acc + torch.mm(a, b)
        out[s].copy_(acc)


def gemm_call(device, kind, A, B, P, S):
    """B: [N, K], or the three planes [3, N, K] for bf16x6."""
    if is_gpu(device):
        g = torch.ops.gksgd
        (g.lstm_rec_gemm_x6 if kind == "x6" else g.lstm_rec_gemm)(A, B, P, S)
    else:
        (mirror_rec_gemm_x6 if kind == "x6" else mirror_rec_gemm)(A, B, P, S)


def _gemm_dense(device, c):
    P = torch.full((c.S, c.M, c.N), NAN, device=device)
    gemm_call(device, c.kind, c.A.to(device), (c.B3 if c.kind == "x6" else c.B).to(device), P, c.S)
    return P


def _gname(c):
    return "M=%d N=%d ks=%d S=%d D=%d trips=%d" % ((c.M, c.N, c.ks, c.S) + rec_variant(c.kind, c.ks))


def scenario_gemm_exact(device, kind):
    t = Tally("R gemm %s exact" % kind)
    for row in GEMM_CASES[kind]:
        c = gemm_case(kind, *row, "exact")
        P = _c64(_gemm_dense(device, c))
        for s in range(c.S):
            d = (P[s] - c.ref[s]).abs()
            t._rec(_gname(c), "P[%d]" % s, "bit-equal", *t._ratio(d, torch.zeros_like(d)), 1.0)
    t.finish()


def scenario_gemm_random(device, kind):
    t = Tally("R gemm %s random" % kind)
    for row in GEMM_CASES[kind]:
        c = gemm_case(kind, *row, "random")
        P = _c64(_gemm_dense(device, c))
        n = {"bf16": c.ks, "fp32": c.ks + 1, "x6": 6 * c.ks + 1}[kind]
        for s in range(c.S):
            t.fp32_sum(_gname(c), "P[%d]" % s, P[s], c.ref[s], n, c.sumabs[s])
            if kind == "x6":
                e = NAN if torch.isnan(P[s]).any() else float((P[s] - c.ref[s]).norm() / c.ref[s].norm())
                t._rec(_gname(c), "P[%d] rel-fro" % s, "yardstick", e, c.yard[s], e / c.yard[s], FACTOR)
    t.finish()


def _window(x, off, device):
    """``x`` [..., R, K] as a column window of a wider, taller NaN-filled buffer: row stride K + 24 elements,
    window offset ``off`` elements (16 bytes), two more rows per plane."""
    K = x.shape[-1]
    buf = torch.full(tuple(x.shape[:-2]) + (x.shape[-2] + 2, K + 24), NAN, dtype=x.dtype, device=device)
    w = buf[..., :x.shape[-2], off:off + K]
    w.copy_(x)
    return w


def scenario_gemm_strided(device, kind):
    """lda / ldb = K + 24, plane stride (N + 2)(K + 24), P inside a sentinel-guarded flat buffer: bit-equal to
    the dense call (an over-read would put NaN into P), nothing stored outside P."""
    t = Tally("R gemm %s strided" % kind)
    for row in GEMM_CASES[kind]:
        c = gemm_case(kind, *row, "random")
        dense = _gemm_dense(device, c)
        A = _window(c.A, 8 if kind == "bf16" else 4, device)
        B = _window(c.B3 if kind == "x6" else c.B, 8, device) if kind != "fp32" else _window(c.B, 4, device)
        assert A.stride(0) == c.K + 24 and B.stride(-2) == c.K + 24 and not B.is_contiguous()
        assert kind != "x6" or B.stride(0) == (c.N + 2) * (c.K + 24)
        n = c.S * c.M * c.N
        flat = torch.full((n + 2 * GUARD,), SENTINEL, device=device)
        P = flat[GUARD:GUARD + n].view(c.S, c.M, c.N)
        P.fill_(NAN)
        gemm_call(device, kind, A, B, P, c.S)
        t.true(_gname(c), "strided operands: P differs from the dense call", torch.equal(P, dense))
        t.true(_gname(c), "a store outside P", bool((flat[:GUARD] == SENTINEL).all()) and
               bool((flat[GUARD + n:] == SENTINEL).all()))
    t.finish()


def gemm_refusals(device, kind):
    """(what, A, B, P, S) of every call that the binding must refuse; the first entry is the accepted base."""
    M, N, K, S = 4, 64, 128, 2
    adt = BF16 if kind == "bf16" else F32
    bdt = F32 if kind == "fp32" else BF16
    ael, bel = (8 if adt == BF16 else 4), (8 if bdt == BF16 else 4)     # elements per 16 bytes
    lead = (3,) if kind == "x6" else ()

    def z(shape, dt):
        return torch.zeros(shape, dtype=dt, device=device)

    def mkA(m=M, k=K, dt=adt):
        return z((m, k), dt)

    def mkB(n=N, k=K, dt=bdt, planes=lead):
        return z(planes + (n, k), dt)

    def mkP(s=S, m=M, n=N):
        return torch.full((s, m, n), SENTINEL, device=device)

    out = [("accepted", mkA(), mkB(), mkP(), S),
           ("K % (64 S) != 0", mkA(), mkB(), mkP(s=3), 3),
           ("K % 64 != 0", mkA(k=96), mkB(k=96), mkP(s=1), 1),
           ("S = 0", mkA(), mkB(), mkP(), 0),
           ("N % 64 != 0", mkA(), mkB(n=32), mkP(n=32), S),
           ("A row stride not 16-byte aligned", mkA(k=K + ael // 2)[:, :K], mkB(), mkP(), S),
           ("B row stride not 16-byte aligned", mkA(), mkB(k=K + bel // 2)[..., :K], mkP(), S),
           ("A base pointer off by one element", mkA(k=K + ael)[:, 1:1 + K], mkB(), mkP(), S),
           ("B base pointer off by one element", mkA(), mkB(k=K + bel)[..., 1:1 + K], mkP(), S),
           ("A column stride 2", mkA(k=2 * K)[:, ::2], mkB(), mkP(), S),
           ("mixed dtypes: A", mkA(dt=F32 if adt == BF16 else BF16), mkB(), mkP(), S),
           ("mixed dtypes: B", mkA(), mkB(dt=F32 if bdt == BF16 else BF16), mkP(), S),
           ("K of A and B differ", mkA(), mkB(k=2 * K), mkP(), S),
           ("P.numel() too large", mkA(), mkB(), mkP(n=N + 64), S),
           ("P.numel() too small", mkA(), mkB(), mkP(s=S - 1), S),
           ("P not fp32", mkA(), mkB(), mkP().double(), S),
           ("P not contiguous", mkA(), mkB(), mkP(n=2 * N)[:, :, ::2], S)]
    if kind == "x6":
        out += [("B3.size(0) != 3", mkA(), mkB(planes=(2,)), mkP(), S),
                ("B3 two-dimensional", mkA(), mkB(planes=()), mkP(), S),
                ("B3 plane stride not 16-byte aligned", mkA(), z((3, N * K + 4), BF16)[:, :N * K].view(3, N, K),
                 mkP(), S)]
    else:
        out += [("B three-dimensional", mkA(), mkB(planes=(3,)), mkP(), S)]
    return out


def scenario_gemm_refusals(device, kind):
    t = Tally("R gemm %s refusals" % kind)
    for what, A, B, P, S in gemm_refusals(device, kind):
        before = P.clone()
        try:
            gemm_call(device, kind, A, B, P, S)
            raised = False
        except RuntimeError:
            raised = True
        if what == "accepted":
            t.true(what, "the base call was refused or wrote no zeros", not raised and not P.any())
        else:
            t.true(what, "not refused", raised)
            t.true(what, "P was written", torch.equal(P, before))
    t.finish()


# --------------------------------------------------------------------------- C. the cell kernels

# (B, H, Hp - pad64(H), S)
CELL_CASES = [(1, 1, 0, 1), (1, 64, 0, 3), (1, 65, 0, 1), (3, 40, 64, 3), (1, 256, 0, 1), (1, 257, 0, 3),
              (5, 63, 0, 3), (129, 3, 0, 1)]
POOL_CASE = (64, 320, 0, 3)
POOL = POOL_CASE[:2]
FWD_PATHS = ("P", "hg", "both")
BWD_SHAPE = (5, 63, 0, 3)
BWD_COMBOS = list(itertools.product((True, False), repeat=4))       # dout, dh_rec, P, dc_next present
SAT_PRE = (20.0, 88.0, 89.0, 104.0, 9984.0)                         # +-: every one exact in bf16
SAT_C = (0.0, 20.0, -20.0, 9984.0, -9984.0)


def fwd_math(a, cp):
    """The forward of the header of lstm.hip on pre-activations ``a`` [B, 4H], in the dtype of ``a``."""
    i, f, g, o = a.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * cp + i * g
    return dict(c=c, h=o * torch.tanh(c), gates=torch.cat([i, f, g, o], dim=1))


def bwd_math(dh, dcn, gates, c, cp):
    """The backward of the header of lstm.hip, in the dtype of ``dh``; ``dcn`` may be None."""
    i, f, g, o = gates.chunk(4, dim=1)
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc)
    if dcn is not None:
        dc = dcn + dc
    dG = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=1)
    return dict(dG=dG, dc_prev=dc * f)


def _split_parts(x, S, gen):
    """A random-weight split of fp32 ``x`` into S stored fp32 slices (the reference sums the stored slices)."""
    w = torch.rand((S,) + tuple(x.shape), generator=gen) + 0.1
    return (x[None] * (w / w.sum(0))).contiguous()


def _total(terms, dt):
    """Sum of the stored terms in the kernel's order: exact in fp64, one rounding per addition in fp32."""
    a = terms[0].to(dt)
    for x in terms[1:]:
        a = a + x.to(dt)
    return a


@functools.lru_cache(maxsize=None)
def cell_inputs(B, H, cd, S, sat=False):
    """Forward and backward operands of one case as stored.  ``sat``: B = 500, H = 100 with every combination
    of the saturating pre-activations of the four gates and of c_prev (unit j: gates i, f; row b: g, o, c_prev)."""
    gen = torch.Generator().manual_seed(B * 1009 + H * 13 + S + (5 if cd == BF16 else 0))
    if sat:
        v = torch.tensor([s * x for x in SAT_PRE for s in (1.0, -1.0)])
        assert (B, H) == (5 * len(v) ** 2, len(v) ** 2) and torch.equal(v.to(BF16).float(), v)
        j, b = torch.arange(H), torch.arange(B)
        xg = torch.stack([v[j // 10].expand(B, H), v[j % 10].expand(B, H), v[b % 10][:, None].expand(B, H),
                          v[(b // 10) % 10][:, None].expand(B, H)], dim=1).reshape(B, 4 * H).to(cd)
        hg = torch.zeros(B, 4 * H).to(cd)
        cp = torch.tensor(SAT_C)[b // 100][:, None].expand(B, H).contiguous()
    else:
        xg = (2 * torch.randn(B, 4 * H, generator=gen)).to(cd)
        hg = torch.randn(B, 4 * H, generator=gen).to(cd)
        cp = torch.randn(B, H, generator=gen)
    n = SimpleNamespace(B=B, H=H, cd=cd, S=S, sat=sat, xg=xg, hg=hg, cp=cp)
    n.parts = _split_parts(hg.float(), S, gen)                       # [S, B, 4H] fp32
    # backward: the state is the fp64 forward of xg + hg, rounded once to the stored fp32
    st = fwd_math(xg.double() + hg.double(), cp.double())
    n.gates, n.c = st["gates"].float(), st["c"].float()
    n.dout = torch.randn(B, H, generator=gen).to(cd)
    n.dh_rec = torch.randn(B, H, generator=gen).to(cd)
    n.dcn = torch.randn(B, H, generator=gen)
    n.dparts = _split_parts(torch.randn(B, H, generator=gen), S, gen)   # [S, B, H] fp32
    return n


def _fwd_terms(n, path):
    return [n.xg] + ([n.hg] if path in ("hg", "both") else []) + (list(n.parts) if path in ("P", "both") else [])


def _bwd_terms(n, combo):
    dout, dh_rec, P, _ = combo
    return ([n.dout] if dout else []) + ([n.dh_rec] if dh_rec else []) + (list(n.dparts) if P else []) or \
        [torch.zeros(n.B, n.H)]


@functools.lru_cache(maxsize=None)
def cell_fwd_refs(B, H, cd, S, path, sat=False):
    """(inputs, fp64 reference, fp32 PyTorch composition) of the forward."""
    n = cell_inputs(B, H, cd, S, sat)
    t = _fwd_terms(n, path)
    return n, fwd_math(_total(t, F64), n.cp.double()), fwd_math(_total(t, F32), n.cp)


@functools.lru_cache(maxsize=None)
def cell_bwd_refs(B, H, cd, S, combo, sat=False):
    n = cell_inputs(B, H, cd, S, sat)
    t = _bwd_terms(n, combo)
    dcn = n.dcn if combo[3] else None
    r64 = bwd_math(_total(t, F64), dcn.double() if combo[3] else None, n.gates.double(), n.c.double(), n.cp.double())
    return n, r64, bwd_math(_total(t, F32), dcn, n.gates, n.c, n.cp)


def _yards(r64, r32):
    return {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}


@functools.lru_cache(maxsize=None)
def fwd_yard(cd, S, path):
    """Rule 3: the yardsticks of the pool case of this storage type, slice count and path."""
    _, r64, r32 = cell_fwd_refs(*POOL, cd, S, path)
    return _yards(r64, r32)


@functools.lru_cache(maxsize=None)
def bwd_yard(cd, S, combo):
    _, r64, r32 = cell_bwd_refs(*POOL, cd, S, combo)
    return _yards(r64, r32)


def _padded_P(parts, cols, Hp, device):
    """[S + 1, B, cols * Hp]: the S slices in the 64-padded gate columns; NaN in the pad columns j >= H and in
    the whole extra slab.  (Hp is a multiple of 64, so the storage offset of P is even whatever B and H.)"""
    S, B = parts.shape[:2]
    H = parts.shape[2] // cols
    P = torch.full((2, S + 1, B, cols, Hp), NAN, device=device)[1]      # the [1] slice, as every operand
    P[:S, :, :, :H] = parts.view(S, B, cols, H).to(device)
    return P.view(S + 1, B, cols * Hp)


def cell_fwd_run(device, n, path, extra=0, pad=True):
    """lstm_cell_fwd on the GPU, ``_cell_fwd_ref`` plus the padded copy elsewhere.  Every operand is the [1]
    slice of a [2, ...] tensor, every output the middle of a sentinel-filled [3, ...] buffer.  Returns the
    outputs, h_pad ([B, Hp], pre-filled with the sentinel) and whether the neighbouring slices are intact."""
    B, H, cd = n.B, n.H, n.cd
    Hp = pad64(H) + (extra if path != "hg" else 0)       # without P the binding takes Hp = pad64(H)
    xg, cp = at1(n.xg, device), at1(n.cp, device)
    hg = at1(n.hg, device) if path in ("hg", "both") else None
    P = _padded_P(n.parts, 4, Hp, device) if path in ("P", "both") else None
    (c, cb), (h, hb), (gates, gb) = out1((B, H), F32, device), out1((B, H), cd, device), out1((B, 4 * H), F32, device)
    h_pad, pb = out1((B, Hp), cd, device) if pad else (None, None)
    if is_gpu(device):
        torch.ops.gksgd.lstm_cell_fwd(xg, hg, P, n.S if P is not None else 0, cp, c, h, h_pad, gates)
    else:
        from gaussiank_sgd_amd.ops.lstm import _cell_fwd_ref
        # the fallback adds two operands: the terms are folded in the kernel's order, the last one is its hg
        terms = [xg] + ([hg] if hg is not None else []) + (list(n.parts) if P is not None else [])
        last = terms.pop() if len(terms) > 1 else torch.zeros(B, 4 * H)
        _cell_fwd_ref(_total(terms, F32), last, cp, c, h, gates)
        if pad:
            h_pad[:, :H] = h
    intact = all(bool((b[0] == SENTINEL).all()) and bool((b[2] == SENTINEL).all()) for b in (cb, hb, gb, pb)
                 if b is not None)
    return dict(c=c, h=h, gates=gates), h_pad, intact


def cell_bwd_run(device, n, combo, extra=0, pad=True):
    B, H, cd = n.B, n.H, n.cd
    Hp = pad64(H) + (extra if combo[2] else 0)
    dout = at1(n.dout, device) if combo[0] else None
    dh_rec = at1(n.dh_rec, device) if combo[1] else None
    P = _padded_P(n.dparts, 1, Hp, device) if combo[2] else None
    dcn = at1(n.dcn, device) if combo[3] else None
    gates, c, cp = at1(n.gates, device), at1(n.c, device), at1(n.cp, device)
    (dG, gb), (dcp, cb) = out1((B, 4 * H), cd, device), out1((B, H), F32, device)
    dG_pad, pb = out1((B, 4 * Hp), cd, device) if pad else (None, None)
    if is_gpu(device):
        torch.ops.gksgd.lstm_cell_bwd(dout, dh_rec, P, n.S if P is not None else 0, dcn, gates, c, cp, dG, dG_pad, dcp)
    else:
        from gaussiank_sgd_amd.ops.lstm import _cell_bwd_ref
        terms = ([dout] if combo[0] else []) + ([dh_rec] if combo[1] else []) + (list(n.dparts) if combo[2] else [])
        last = terms.pop() if terms else None
        _cell_bwd_ref(_total(terms, F32) if terms else None, last, dcn, gates, c, cp, dG, dcp)
        if pad:
            dG_pad.view(B, 4, Hp)[:, :, :H] = dG.view(B, 4, H)
    intact = all(bool((b[0] == SENTINEL).all()) and bool((b[2] == SENTINEL).all()) for b in (gb, cb, pb)
                 if b is not None)
    return dict(dG=dG, dc_prev=dcp), dG_pad, intact


def _cell_check(t, case, cd, ours, r64, Y, stored):
    """fp32 tensors on the yardstick, the bf16-stored one (``stored``: h or dG) on rule 1."""
    for k in r64:
        t.true(case, "%s: dtype / shape" % k, ours[k].dtype == (cd if k == stored else F32) and
               ours[k].shape == r64[k].shape)
        t.true(case, "%s is not finite" % k, bool(torch.isfinite(ours[k].float()).all()))
        if k == stored and cd == BF16:
            t.bf16_out(case, k, ours[k], r64[k], FACTOR * Y[k])
        else:
            yard_abs(t, case, k, ours[k], r64[k], Y[k])


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def scenario_cell_fwd(device, cd):
    """Every shape (and the pool case) on every forward path, with the padded copy."""
    t = Tally("C cell fwd " + cdname(cd))
    for B, H, extra, S in CELL_CASES + [POOL_CASE]:
        for path in FWD_PATHS:
            n, r64, _ = cell_fwd_refs(B, H, cd, S, path)
            case = "B=%d H=%d Hp=%d S=%d %s" % (B, H, pad64(H) + extra, S, path)
            ours, h_pad, intact = cell_fwd_run(device, n, path, extra)
            _cell_check(t, case, cd, ours, r64, fwd_yard(cd, S, path), "h")
            t.true(case, "a store outside c / h / gates / h_pad", intact)
            t.true(case, "h_pad[:, :H] differs from h", torch.equal(h_pad[:, :H], ours["h"]))
            t.true(case, "pad columns of h_pad were written", bool((h_pad[:, H:].float() == SENTINEL).all()))
            again, h_pad2, _ = cell_fwd_run(device, n, path, extra)
            t.true(case, "two runs differ", _same(ours, again) and torch.equal(h_pad, h_pad2))
            plain, none, _ = cell_fwd_run(device, n, path, extra, pad=False)
            t.true(case, "the run without h_pad differs", none is None and _same(ours, plain))
    t.finish()


def _dG_pad_checks(t, case, dG_pad, dG, B, H):
    v = dG_pad.view(B, 4, -1)
    t.true(case, "dG_pad gate blocks differ from dG", torch.equal(v[:, :, :H], dG.view(B, 4, H)))
    t.true(case, "pad columns of dG_pad were written", bool((v[:, :, H:].float() == SENTINEL).all()))


def scenario_cell_bwd(device, cd):
    """Every shape with all four operands; every present / absent combination of them at one shape."""
    t = Tally("C cell bwd " + cdname(cd))
    full = (True, True, True, True)
    rows = [(r, full) for r in CELL_CASES + [POOL_CASE]] + [(BWD_SHAPE, cb) for cb in BWD_COMBOS if cb != full]
    for (B, H, extra, S), combo in rows:
        n, r64, _ = cell_bwd_refs(B, H, cd, S, combo)
        case = "B=%d H=%d Hp=%d S=%d %s" % (B, H, pad64(H) + extra, S, "".join(
            ch if on else "-" for ch, on in zip(("o", "r", "P", "c"), combo)))
        ours, dG_pad, intact = cell_bwd_run(device, n, combo, extra)
        _cell_check(t, case, cd, ours, r64, bwd_yard(cd, S, combo), "dG")
        t.true(case, "a store outside dG / dc_prev / dG_pad", intact)
        _dG_pad_checks(t, case, dG_pad, ours["dG"], B, H)
        again, dG_pad2, _ = cell_bwd_run(device, n, combo, extra)
        t.true(case, "two runs differ", _same(ours, again) and torch.equal(dG_pad, dG_pad2))
        plain, none, _ = cell_bwd_run(device, n, combo, extra, pad=False)
        t.true(case, "the run without dG_pad differs", none is None and _same(ours, plain))
        if not any(combo):
            t.true(case, "no incoming gradient: dG and dc_prev must be exactly zero",
                   not ours["dG"].float().any() and not ours["dc_prev"].any())
    t.finish()


SAT_SHAPE = (500, 100)


def scenario_cell_saturation(device, cd):
    """Pre-activations of +-20 .. +-9984 and c_prev up to +-9984: finite, within the rules -- the yardstick is
    the fp32 composition on the case itself, 50000 elements with every combination, a pool of its own input
    distribution -- and exactly zero wherever the fp64 backward on the stored gates is exactly zero."""
    t = Tally("C cell saturation " + cdname(cd))
    B, H = SAT_SHAPE
    n, r64, r32 = cell_fwd_refs(B, H, cd, 1, "none", True)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    ours, _, intact = cell_fwd_run(device, n, "none", pad=False)
    _cell_check(t, "fwd", cd, ours, r64, _yards(r64, r32), "h")
    t.true("fwd", "a store outside c / h / gates", intact)
    assert bool((n.gates == 1).any()) and bool((n.gates == 0).any())
    assert bool((torch.tanh(n.c.double()).abs() == 1).any())
    for combo in ((True, True, True, True), (True, False, False, False)):
        n, b64, b32 = cell_bwd_refs(B, H, cd, 1, combo, True)
        case = "bwd" + ("" if combo[3] else " without dc_next")
        ours, _, intact = cell_bwd_run(device, n, combo, pad=False)
        _cell_check(t, case, cd, ours, b64, _yards(b64, b32), "dG")
        t.true(case, "a store outside dG / dc_prev", intact)
        for k in b64:
            zero = (b64[k] == 0)
            assert bool(zero.any())
            t.true(case, "%s: nonzero where the fp64 backward is exactly zero" % k,
                   not ours[k].float().cpu()[zero].any())
    t.finish()


def cell_refusals(device, cd):
    """(what, op, args) of calls that lstm_cell_fwd / lstm_cell_bwd must refuse (GPU only); first the accepted
    bases."""
    B, H, Hp, S = 3, 40, 64, 2
    other = F32 if cd == BF16 else BF16

    def z(*shape, dt=F32):
        return torch.zeros(shape, dtype=dt, device=device)

    def fwd(xg=None, hg=None, P=None, S=S, cp=None, c=None, h=None, h_pad=None, gates=None):
        d = lambda v, mk: mk() if v is None else (None if v is False else v)  # noqa: E731
        return (d(xg, lambda: z(B, 4 * H, dt=cd)), d(hg, lambda: None), d(P, lambda: z(S, B, 4 * Hp)), S,
                d(cp, lambda: z(B, H)), d(c, lambda: z(B, H)), d(h, lambda: z(B, H, dt=cd)),
                d(h_pad, lambda: z(B, Hp, dt=cd)), d(gates, lambda: z(B, 4 * H)))

    def bwd(dout=None, P=None, S=S, dcn=None, gates=None, c=None, dG=None, dG_pad=None, dcp=None):
        d = lambda v, mk: mk() if v is None else (None if v is False else v)  # noqa: E731
        return (d(dout, lambda: z(B, H, dt=cd)), None, d(P, lambda: z(S, B, Hp)), S, d(dcn, lambda: z(B, H)),
                d(gates, lambda: z(B, 4 * H)), d(c, lambda: z(B, H)), z(B, H), d(dG, lambda: z(B, 4 * H, dt=cd)),
                d(dG_pad, lambda: z(B, 4 * Hp, dt=cd)), d(dcp, lambda: z(B, H)))

    return [("accepted", "fwd", fwd()), ("accepted", "bwd", bwd()),
            ("hg of the other storage type", "fwd", fwd(hg=z(B, 4 * H, dt=other))),
            ("h of the other storage type", "fwd", fwd(h=z(B, H, dt=other))),
            ("h_pad of the other storage type", "fwd", fwd(h_pad=z(B, Hp, dt=other))),
            ("S > P.size(0)", "fwd", fwd(S=S + 1, P=z(S, B, 4 * Hp))),
            ("P with Hp no multiple of 64", "fwd", fwd(P=z(S, B, 4 * 48))),
            ("P with Hp < H", "fwd", fwd(xg=z(B, 4 * 65, dt=cd), cp=z(B, 65), c=z(B, 65), h=z(B, 65, dt=cd),
                                        gates=z(B, 4 * 65), h_pad=False)),
            ("P with another batch size", "fwd", fwd(P=z(S, B + 1, 4 * Hp))),
            ("h_pad narrower than Hp", "fwd", fwd(h_pad=z(B, H, dt=cd))),
            ("xg not contiguous", "fwd", fwd(xg=z(B, 8 * H, dt=cd)[:, ::2])),
            ("c of another size", "fwd", fwd(c=z(B, H + 1))),
            ("gates not fp32", "fwd", fwd(gates=z(B, 4 * H, dt=BF16))),
            ("dout of the other storage type", "bwd", bwd(dout=z(B, H, dt=other))),
            ("dG_pad of the other storage type", "bwd", bwd(dG_pad=z(B, 4 * Hp, dt=other))),
            ("S > P.size(0)", "bwd", bwd(S=S + 1, P=z(S, B, Hp))),
            ("P with Hp no multiple of 64", "bwd", bwd(P=z(S, B, 48))),
            ("dG_pad narrower than 4 Hp", "bwd", bwd(dG_pad=z(B, 4 * H, dt=cd))),
            ("dc_next not fp32", "bwd", bwd(dcn=z(B, H, dt=BF16))),
            ("gates not contiguous", "bwd", bwd(gates=z(B, 8 * H)[:, ::2])),
            ("dc_prev of another size", "bwd", bwd(dcp=z(B, H + 1)))]


def scenario_cell_refusals(device, cd):
    assert is_gpu(device)
    g = torch.ops.gksgd
    t = Tally("C cell refusals " + cdname(cd))
    for what, op, args in cell_refusals(device, cd):
        try:
            (g.lstm_cell_fwd if op == "fwd" else g.lstm_cell_bwd)(*args)
            raised = False
        except RuntimeError:
            raised = True
        t.true("%s %s" % (op, what), "refused" if what == "accepted" else "not refused", raised != (what == "accepted"))
    t.finish()
