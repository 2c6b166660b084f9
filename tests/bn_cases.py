"""Shared cases of the BatchNorm streaming-kernel tests (csrc/kernels/bn_act.hip: stats, finalize, apply,
BN + ReLU + max-pool, backward reduce / finalize / apply, the pool gather and the pool tile kernel).
tests/test_bn_edges_cpu.py runs them through ``BNAct``'s PyTorch fallback, tests/test_bn_edges_gpu.py on the
HIP kernels (through ``BNAct`` where it reaches the path, through the raw ops where it does not).  Every
reference is fp64 on the CPU, on the inputs as stored, written out from the formulas (no autograd):

    mean, var (biased), invstd = 1 / sqrt(var + eps), xhat = (x - mean) invstd, z = gamma xhat + beta [+ res]
    y = relu(z) [max-pooled];  dz = gated / gathered (dy [+ dy2])
    dbeta = sum dz, dgamma = sum dz xhat, dx = gamma invstd (dz - dbeta / M - xhat dgamma / M), dres = dz

Geometry mirror
---------------
``bn_geo(M, C, elem_bytes, blocks)`` writes out ``make_geo`` of bn_act.hip; the GPU test holds it against
``bn_workspace_floats`` for every shape used here.  ``assert_case_table()`` asserts from the mirror that each
case reaches the property it exists for (rows per thread >= 3, tpr == 1, C < 16, idle lanes, an empty
trailing workgroup, tile / WM=2 / WM=0 gather, KK=3 / runtime-k forward, several tiles per pool thread).

Tolerance rules
---------------
No rule looks at the output under test to size itself.  u = 2^-24; D = ceil(rows_b / rl) + 1 counts the fp32
roundings behind one partial (a thread's rows in fp32; the rl lane sums are added in fp64 and rounded once to
the fp32 partial); the finalize adds the gy partials in fp64.

A channel is a YARDSTICK channel when its statistics are well conditioned, kappa =
(E[x^2] + 2 |mean| E|x|) / (2 (var + eps)) <= 2 (0.5 for a standard normal; (mean / std)^2 <~ 1), else an
OFFSET channel -- decided from the fp64 reference; an offset case has at least one.  Every channel of the N
cases at mean 4, 16 and 100 is one, a constant channel is one, and so are some channels of the M = 2 and
M = 3 cases: with two or three values a channel's sample mean is large against its sample deviation by
chance, and the one-pass variance loses (mean / std)^2 there like anywhere else.  The rule-2 terms below
are added for the offset channels alone; the other channels of the same tensor stay on the yardstick.

1. partials (``Tally.fp32_sum``): |ours - ref| <= D 2^-23 sum|terms| per workgroup and channel, the terms
   being the block's x and x^2 (one fma per square: one rounding per step); a workgroup without rows gives 0.
2. statistics, with D of the deepest block:
     |d mean| <= D 2^-23 E|x| + 2^-24 |mean|
     |d var|  <= D 2^-23 (E[x^2] + 2 |mean| E|x|)           (q / M - mean^2, one pass)
     invstd   relative |d var| / (2 (var + eps)) + 2^-23, written exactly: with r = |d var| / (var + eps),
              1 / sqrt(1 - r) - 1 (= r / 2 to first order; no bound when r >= 1)
   running_mean / running_var carry momentum times these (var times M / (M - 1)) plus three fp32 roundings
   of the update per step.  The N cases at std 1 assert from the reference that the invstd bound is
   <= 1e-2, so it is never vacuous there; (100, 0.1) shows where it is.
3. dbeta / dgamma: D 2^-23 sum|terms| + 2^-24 |ref| (the finalize's rounding); the terms are |dz| and
   |dz xhat| (D + 2 for dgamma: xhat is formed with two roundings), and dgamma adds what rule 2 lets xhat
   move by: sum|dz| (|xhat| (rel_invstd + 3u) + invstd |d mean|).  With D = rows / rl + 1 that term is of
   the order of the sum's own (at M = 3 a gated dz leaves one or two terms, and the rounding of invstd
   alone exceeds D 2^-23 sum|dz xhat|); the whole stays far below the bound of a chain over the rl lanes.
4. y, dx (the bound is printed with FACTOR folded in; limit 1):
     fp32 storage: FACTOR x the max error of the fp32 PyTorch CPU composition against fp64 (the yardstick);
     bf16 storage: elementwise 2^-8 |ref| + E with E = that bound on the bf16 values (``bf16-out``);
     offset channels add, elementwise, |gamma| invstd (rel_invstd |x - mean| + |d mean|) to y and the
     first-order image of rule 2 and rule 3 to dx; the plain yardstick ratio of such a case is printed, not
     asserted.
   dres is dz itself and must be exact (the gradients here lie on a 1/16 grid, so dy + dy2 is exact).
5. decisions (ReLU gate, pool argmax): the fp64 reference is evaluated with the decisions of the output it
   is compared with (gate = y > 0; the argmax bytes).  First those decisions must equal the fp64 ones
   wherever the fp64 margin exceeds E of rule 4 (|z| for the gate and the blocked-window flag; the top-2
   gap of a window for fp32 storage).  bf16 storage compares bf16-rounded values, where ties are common
   and legitimate (first maximum wins, as in the kernel and in at::max_pool2d): a window is undecided when
   a contender (rounded value within two bf16 steps of the top) lies within E of a rounding midpoint.
   In an offset channel the margin of the gate is the bound of rule 4 with its rule-2 term.  Undecided
   elements may number at most 0.1 % of a tensor (one element in a tensor of fewer than 1000), in every
   case but (100, 0.1), where rule 2 gives no bound and every element is undecided.
6. bitwise: twin (dy, dy2) equals the single gradient dy + dy2; two runs of one configuration are
   bit-identical; 64 and the default number of workgroups are each held to rules 1-4 (not to equality).

Every check prints ``TOL | family | case | tensor | rule | err | bound | ratio``;
profiles/bn_kernels_tolerances.txt is the worst line per family and tensor of the GPU run.
"""
import functools
import math
import os
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import bert_row_cases as rc
from bert_row_cases import BF16, BF16_ULP, F32, F64, FACTOR, FP32_SUM, Tally, is_gpu

EPS = 1e-5
MOM = 0.1
U24 = 2.0 ** -24
CL = torch.channels_last
BLOCK = 256            # kBlock
MIN_BLOCKS = 64        # lower clamp of bn_set_blocks
POOL_BLOCKS = 4096     # kPoolTargetBlocks (also the grid the workspace is sized for)
UNDECIDED_CAP = 1e-3


def default_blocks():
    return int(os.environ.get("GKSGD_BN_BLOCKS", 1024))


def cdname(cd):
    return "bf16" if cd == BF16 else "fp32"


def ebytes(cd):
    return 2 if cd == BF16 else 4


# --------------------------------------------------------------------------- geometry mirror

def bn_geo(M, C, elem_bytes, blocks):
    """make_geo of bn_act.hip written out."""
    V = 8 if elem_bytes == 2 else 4
    assert C % V == 0 and C >= V and M >= 1
    cv = C // V
    tpr = max(d for d in range(1, min(cv, 64) + 1) if cv % d == 0)
    rl = BLOCK // tpr
    gx = C // (tpr * V)
    gy = max(1, min(-(-blocks // gx), -(-M // rl)))
    rpb = -(-M // gy)
    return SimpleNamespace(M=M, C=C, V=V, tpr=tpr, rl=rl, gx=gx, gy=gy, rpb=rpb)


def block_rows(g):
    return [max(0, min(g.M, (b + 1) * g.rpb) - b * g.rpb) for b in range(g.gy)]


def depth(g, rows=None):
    """fp32 roundings behind a partial of a block with ``rows`` rows (default: the fullest): a thread's rows,
    then the one rounding of the fp64 sum of the rl lane sums."""
    rows = g.rpb if rows is None else rows
    return -(-rows // g.rl) + 1


def rows_per_thread(g):
    """(fewest, most) rows a working lane of the fullest block walks."""
    return g.rpb // g.rl, -(-g.rpb // g.rl)


def idle_lanes(g):
    return BLOCK - g.tpr * g.rl


def empty_blocks(g):
    return sum(1 for r in block_rows(g) if r == 0)


def pool_out(H, W, pool):
    k, s, p = pool
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def pool_path(pool):
    """Which backward gather bn_pool_backward_tw takes."""
    k, s, p = pool
    if s == 2 and k <= 4:
        return "tile"
    return "wm2" if -(-k // s) <= 2 else "wm0"


def pool_fwd(pool):
    return "kk3" if pool[0] == 3 and pool[2] == 1 else "runtime"


def pool_tiles(shape, pool):
    N, _, H, W = shape
    k, s, p = pool
    return N * ((H + p + s - 1) // s) * ((W + p + s - 1) // s)


def pool_uncovered(H, pool):
    """Trailing input rows that no window reaches."""
    k, s, p = pool
    return H - 1 - min(H - 1, (pool_out(H, H, pool)[0] - 1) * s - p + k - 1)


# --------------------------------------------------------------------------- the case tables

Variant = namedtuple("Variant", "relu res twin")
VARIANTS = {"bn": Variant(False, False, False), "relu": Variant(True, False, False),
            "res_relu": Variant(True, True, False), "twin": Variant(True, False, True),
            "twin_res": Variant(True, True, True)}

# G: name -> (fp32 shape, bf16 shape, the workgroups at which the property holds (None: the default), the
# property asserted from the mirror); every case RUNS at 64 and at the default (g_blocks)
G_CASES = {
    "multirow": ((8, 64, 28, 28), (8, 64, 28, 28), MIN_BLOCKS,
                 lambda g, cd: rows_per_thread(g)[0] >= 3 and (cd == BF16 or (g.rl, g.gy, g.rpb) == (16, 64, 98))),
    "prime": ((3, 268, 17, 13), (3, 536, 17, 13), MIN_BLOCKS,
              lambda g, cd: g.tpr == 1 and g.gx == 67 and g.gy == 1 and rows_per_thread(g) == (2, 3)),
    "minc_small": ((2, 4, 9, 11), (2, 8, 9, 11), MIN_BLOCKS,
                   lambda g, cd: g.C < 16 and g.M < g.rl and g.gy == 1),
    "minc_rows": ((4, 4, 67, 67), (4, 8, 67, 67), MIN_BLOCKS,
                  lambda g, cd: g.C < 16 and g.rpb == 281 and rows_per_thread(g) == (1, 2)),
    "idle": ((3, 40, 5, 7), (3, 72, 5, 7), None,
             lambda g, cd: g.C % 16 != 0 and idle_lanes(g) > 0 and (g.tpr, g.rl) == ((10, 25) if cd == F32 else (9, 28))),
    "trailing": ((8, 2048, 5, 25), (8, 4096, 5, 25), None,
                 lambda g, cd: empty_blocks(g) >= 1 and (g.gy - 1) * g.rpb >= g.M and
                 (cd == BF16 or (g.gy, g.rpb) == (128, 8))),
    "m2": ((1, 64, 1, 2), (1, 64, 1, 2), None, lambda g, cd: g.M == 2 and g.M < g.rl),
    "m3": ((1, 64, 3, 1), (1, 64, 3, 1), None, lambda g, cd: g.M == 3 and g.M < g.rl),
}

P_SHAPE = {F32: (2, 8, 13, 10), BF16: (2, 16, 13, 10)}
P_POOLS = {"tile": [(3, 2, 1), (2, 2, 0), (4, 2, 1), (3, 2, 0), (1, 2, 0)],
           "wm2": [(2, 1, 0), (3, 3, 1), (2, 3, 0), (5, 3, 2)],
           "wm0": [(3, 1, 1), (5, 2, 2), (4, 1, 2)]}
# (3, 2, 1) with several tiles per pool thread: gy * rl < ntiles needs ntiles > 2^20 / (C / V) whatever C is
# (16.9 M elements in fp32 and twice that in bf16, with an fp64 reference of each: the case runs in fp32, twin
# off -- the tile loop does not depend on the storage type or on TWIN, which the small shapes cover)
P_MULTITILE = ((2, 268, 178, 178), (3, 2, 1))
# a 1 x 1 image under a padded 4 x 4 / 2 pool has more tiles than pixels (the tile grid must not be used)
P_MORE_TILES_THAN_ROWS = ((300, 4, 1, 1), (4, 2, 2))
N_SHAPE = (8, 64, 28, 28)
N_STATS = [(0.0, 1.0), (4.0, 1.0), (16.0, 1.0), (100.0, 0.1)]
S_SHAPE = {F32: (3, 40, 5, 7), BF16: (3, 72, 5, 7)}


def g_shape(name, cd):
    return G_CASES[name][0 if cd == F32 else 1]


def g_blocks(name):
    """Every geometry case runs at 64 workgroups and at the default (the property of its table row holds at
    the one named there; the other is one more launch geometry of the same shape, e.g. trailing fp32 at 64:
    gy = 8, rows_per_block = 125, rl = 4, 31-32 rows per thread)."""
    return sorted({MIN_BLOCKS, default_blocks()})


def assert_case_table():
    """Every named property, from the mirror."""
    for name, (s32, s16, blocks, prop) in G_CASES.items():
        for cd, (N, C, H, W) in ((F32, s32), (BF16, s16)):
            g = bn_geo(N * H * W, C, ebytes(cd), blocks or default_blocks())
            assert prop(g, cd), (name, cdname(cd), vars(g))
    for path, pools in P_POOLS.items():
        for pool in pools:
            assert pool_path(pool) == path, (pool, path)
    allp = [p for ps in P_POOLS.values() for p in ps]
    assert {pool_fwd(p) for p in allp} == {"kk3", "runtime"}
    assert pool_fwd((3, 3, 1)) == "kk3" and pool_path((3, 3, 1)) == "wm2"          # KK = 3 forward at s != 2
    H, W = P_SHAPE[F32][2:]
    assert P_SHAPE[BF16][2:] == (H, W)
    # the last row or column is uncovered: it gets the BN backward of dz = 0
    assert sum(1 for p in P_POOLS["tile"] if pool_uncovered(H, p) > 0 or pool_uncovered(W, p) > 0) >= 3
    assert pool_uncovered(H, (2, 2, 0)) == 1 and pool_uncovered(W, (3, 2, 0)) == 1
    assert pool_uncovered(13, (2, 3, 0)) > 0 and (2, 3, 0)[1] > (2, 3, 0)[0]        # gaps between the windows
    shape, pool = P_MULTITILE
    g = bn_geo(pool_tiles(shape, pool), shape[1], 4, POOL_BLOCKS)
    assert pool_path(pool) == "tile" and rows_per_thread(g)[1] >= 2, vars(g)
    shape, pool = P_MORE_TILES_THAN_ROWS
    assert pool_tiles(shape, pool) > shape[0] * shape[2] * shape[3]
    g = bn_geo(N_SHAPE[0] * N_SHAPE[2] * N_SHAPE[3], N_SHAPE[1], 4, MIN_BLOCKS)
    assert rows_per_thread(g)[0] >= 3


assert_case_table()


# --------------------------------------------------------------------------- inputs and the fp64 reference

def rows(t):
    """[N, C, H, W] of any layout -> fp64 [M, C] rows on the CPU."""
    return t.detach().to("cpu").permute(0, 2, 3, 1).reshape(-1, t.shape[1]).to(F64)


def nchw(r, shape, dt=None):
    """[M, C] rows -> a channels-last [N, C, H, W] tensor."""
    N, C, H, W = shape
    t = r.reshape(N, H, W, C).permute(0, 3, 1, 2)
    return t if dt is None else t.to(dt)


def _grid(gen, n, c, cd):
    """Gradients on a 1/16 grid in [-4, 4]: exact in bf16 and fp32, and so is the sum of two of them."""
    return ((torch.randn(n, c, generator=gen) * 16).round().clamp(-64, 64) / 16).to(cd)


def _stats(xr, gamma, beta):
    M = xr.shape[0]
    mean = xr.mean(0)
    var = ((xr - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    return SimpleNamespace(M=M, mean=mean, var=var, invstd=invstd, xhat=(xr - mean) * invstd,
                           absmean=xr.abs().mean(0), sqmean=(xr * xr).mean(0))


@functools.lru_cache(maxsize=None)
def bn_inputs(shape, cd, mean=0.0, std=1.0, gamma="pos", affine=True, seed=0, const=None):
    """x, res, dy, dy2 ([N, C, H, W] channels-last, storage dtype ``cd``), gamma / beta (fp32) and the fp64
    statistics of x as stored.  ``gamma``: "pos" in [0.5, 1.5]; "mixed": negative, zero, positive by c % 3.
    ``const``: a channel set to the constant 0.5 (variance exactly 0) among the normal ones.
    ``off`` marks the offset channels (kappa > 2); ``offset``: the case has one."""
    N, C, H, W = shape
    M = N * H * W
    gen = torch.Generator().manual_seed(1000003 * seed + 131 * M + C + (7 if cd == BF16 else 0) + int(10 * mean))
    xr = (mean + std * torch.randn(M, C, generator=gen)).to(cd)
    rr = torch.randn(M, C, generator=gen).to(cd)
    dy, dy2 = _grid(gen, M, C, cd), _grid(gen, M, C, cd)
    if const is not None:
        xr[:, const] = 0.5
    if not affine:
        g, b = torch.ones(C), torch.zeros(C)
    else:
        g = torch.rand(C, generator=gen) + 0.5
        b = torch.rand(C, generator=gen) - 0.5
        if gamma == "mixed":
            g = g * torch.tensor([-1.0, 0.0, 1.0])[torch.arange(C) % 3]
    st = _stats(xr.double(), g.double(), b.double())
    return SimpleNamespace(shape=shape, cd=cd, M=M, C=C, affine=affine, x=nchw(xr, shape), res=nchw(rr, shape),
                           dy=nchw(dy, shape), dy2=nchw(dy2, shape), gamma=g, beta=b, st=st,
                           off=(kappa(st) > KAPPA_YARDSTICK).double(), offset=bool((kappa(st) > KAPPA_YARDSTICK).any()))


def bn_ref(inp, v, gate):
    """The fp64 formulas with the given ReLU gate ([M, C] bool; ignored without ReLU)."""
    st, g, b = inp.st, inp.gamma.double(), inp.beta.double()
    bn = st.xhat * g + b
    z = bn + rows(inp.res) if v.res else bn
    dyt = rows(inp.dy) + (rows(inp.dy2) if v.twin else 0.0)
    if v.relu:
        y, dz = torch.where(gate, z, torch.zeros_like(z)), torch.where(gate, dyt, torch.zeros_like(dyt))
    else:
        y, dz = z, dyt
    return _bn_backward(inp, dict(y=y, z=z, bn=bn, dz=dz))


def _bn_backward(inp, r):
    st, g, dz = inp.st, inp.gamma.double(), r["dz"]
    r["db"], r["dg"] = dz.sum(0), (dz * st.xhat).sum(0)
    r["dx"] = g * st.invstd * (dz - r["db"] / st.M - st.xhat * r["dg"] / st.M)
    r["s_dz"], r["s_dzxhat"] = dz.abs().sum(0), (dz * st.xhat).abs().sum(0)
    return r


def bn_torch(inp, v, dt=F32):
    """The PyTorch CPU composition at ``dt`` (the yardstick at fp32) with autograd; rows out."""
    x = inp.x.to(dt).clone().requires_grad_(True)
    res = inp.res.to(dt).clone().requires_grad_(True) if v.res else None
    w = inp.gamma.clone().requires_grad_(True) if inp.affine else None
    b = inp.beta.clone().requires_grad_(True) if inp.affine else None
    y = F.batch_norm(x, None, None, w, b, True, 0.0, EPS)
    if v.res:
        y = y + res
    if v.relu:
        y = F.relu(y)
    y.backward((inp.dy.to(dt) + inp.dy2.to(dt)) if v.twin else inp.dy.to(dt))
    return dict(y=rows(y), dx=rows(x.grad), dres=rows(res.grad) if v.res else None,
                dg=w.grad.double() if inp.affine else None, db=b.grad.double() if inp.affine else None)


def stat_bounds(inp, D):
    """Rule 2: (|d mean|, |d var|, relative invstd) per channel."""
    st = inp.st
    dmean = D * FP32_SUM * st.absmean + U24 * st.mean.abs()
    dvar = D * FP32_SUM * (st.sqmean + 2 * st.mean.abs() * st.absmean)
    r = dvar / (st.var + EPS)
    rel = torch.where(r < 1, 1 / torch.sqrt((1 - r).clamp(min=1e-300)) - 1, torch.full_like(r, NO_BOUND))
    return dmean, dvar, rel + FP32_SUM


def kappa(st):
    """Conditioning of the one-pass variance per channel: rule 2's |d var| / (2 (var + eps)) per unit D 2^-23."""
    return (st.sqmean + 2 * st.mean.abs() * st.absmean) / (2 * (st.var + EPS))


KAPPA_YARDSTICK = 2.0
NO_BOUND = 1e30          # stat_bounds: the relative invstd bound of a channel with |d var| >= var + eps


def _elem(t, case, name, rule, ours, ref, bound):
    ours, ref = ours.to(F64), ref.to(F64)
    assert ours.shape == ref.shape, (case, name, ours.shape, ref.shape)
    t._rec(case, name, rule, *t._ratio((ours - ref).abs(), bound.expand_as(ref).to(F64)), 1.0)


def _maxerr(a, b):
    return float((a.to(F64) - b.to(F64)).abs().max()) if a.numel() else 0.0


def _undecided(t, case, what, decisive, same, cap=True):
    """Rule 5: ``same`` wherever ``decisive``; the rest at most 0.1 % of the tensor (``cap``)."""
    n = decisive.numel()
    und = int((~decisive).sum())
    print("DEC | %s | %s | %s | undecided %d of %d | decided and different %d" % (
        t.family, case, what, und, n, int((decisive & ~same).sum())))
    t.true(case, "%s: %d decisions differ from fp64 outside the margin" % (what, int((decisive & ~same).sum())),
           bool((same | ~decisive).all()))
    # a tensor of fewer than 1000 elements may hold one
    t.true(case, "%s: %d of %d inside the margin (cap 0.1 %%)" % (what, und, n),
           not cap or und <= max(1.0, UNDECIDED_CAP * n))


def grad_bounds(inp, r, D, dmean, rel_is):
    """Rule 3: bounds of dbeta and dgamma per channel, and what rule 2 lets xhat move by."""
    st = inp.st
    b_db = D * FP32_SUM * r["s_dz"] + U24 * r["db"].abs()
    b_dg = (D + 2) * FP32_SUM * r["s_dzxhat"] + U24 * r["dg"].abs()
    dxhat = st.xhat.abs() * (rel_is + 3 * U24) + st.invstd * dmean
    b_dg = b_dg + (r["dz"].abs() * dxhat).sum(0)
    return b_db, b_dg, dxhat


def bn_check(t, case, ours, inp, v, D, fused, fwd_only=False):
    """Rules 3-5 on y, dx, dres, dgamma, dbeta of one BNAct run (``ours``: [N, C, H, W] tensors and [C]);
    ``fwd_only``: y alone."""
    st, g = inp.st, inp.gamma.double()
    yo = rows(ours["y"])
    gate = yo > 0
    r = bn_ref(inp, v, gate)
    yd = bn_torch(inp, v)
    ry = bn_ref(inp, v, yd["y"] > 0)
    Ey, Edx = FACTOR * _maxerr(yd["y"], ry["y"]), FACTOR * _maxerr(yd["dx"], ry["dx"])
    dmean, dvar, rel_is = stat_bounds(inp, D)
    b_db, b_dg, dxhat = grad_bounds(inp, r, D, dmean, rel_is)
    by, bdx = torch.full_like(r["y"], Ey), torch.full_like(r["dx"], Edx)
    if inp.offset:
        if inp.cd == F32:
            t._rec(case, "y", "yardstick (not asserted)", _maxerr(yo, r["y"]), Ey, _maxerr(yo, r["y"]) / Ey, math.inf)
        by = by + inp.off * g.abs() * st.invstd * (rel_is * (rows(inp.x) - st.mean).abs() + dmean)
        bdx = bdx + inp.off * (r["dx"].abs() * rel_is + g.abs() * st.invstd * (
            b_db / st.M + dxhat * (r["dg"] / st.M).abs() + st.xhat.abs() * b_dg / st.M))
    # the bf16 composition rounds bn(x) to bf16 before it adds the residual (the kernel rounds once, at the
    # end): that rounding can turn the sign of z, so it widens the margin there and the cap is the kernel's
    twice = inp.cd == BF16 and v.res and not fused
    extra = BF16_ULP * (1 + 2.0 ** -7) * r["bn"].abs() if twice else 0.0
    if v.relu:
        # offset channels: the margin is the derived bound.  The cap holds for every case but the one where
        # rule 2 gives no bound at all ((100, 0.1): |d var| >= var + eps), decided from the reference
        _undecided(t, case, "relu gate", r["z"].abs() > by + extra, gate == (r["z"] > 0),
                   cap=not twice and float(rel_is.max()) < NO_BOUND)
    rule = "yardstick" + ("+rule2" if inp.offset else "")
    if inp.cd == BF16:
        by = BF16_ULP * (1 + 2.0 ** -7 if twice else 1.0) * r["y"].abs() + extra + by
        bdx = BF16_ULP * r["dx"].abs() + bdx
        rule = "bf16-out" + ("+rule2" if inp.offset else "")
    t.true(case, "NaN in y", not torch.isnan(yo).any())
    _elem(t, case, "y", rule, yo, r["y"], by)
    t.true(case, "output dtype / layout", ours["y"].dtype == inp.cd and ours["y"].is_contiguous(memory_format=CL))
    if fwd_only:
        return r
    if inp.offset and inp.cd == F32:
        e = _maxerr(rows(ours["dx"]), r["dx"])
        t._rec(case, "dx", "yardstick (not asserted)", e, Edx, e / Edx, math.inf)
    _elem(t, case, "dx", rule, rows(ours["dx"]), r["dx"], bdx)
    t.true(case, "dx dtype", ours["dx"].dtype == inp.cd)
    if v.res:
        t.true(case, "dres must be dz exactly", torch.equal(rows(ours["dres"]), r["dz"]))
    if inp.affine:
        _elem(t, case, "dbeta", "fp32-sum", ours["db"].cpu(), r["db"], b_db)
        _elem(t, case, "dgamma", "fp32-sum+rule2", ours["dg"].cpu(), r["dg"], b_dg)
        zero = inp.gamma == 0
        if bool(zero.any()):
            t.true(case, "gamma == 0 must give dx == 0 exactly", not rows(ours["dx"])[:, zero].any())
    else:
        t.true(case, "affine=False has no parameter gradients", ours["dg"] is None and ours["db"] is None)
    return r


def running_check(t, case, mod, inps, D, momentum=MOM):
    """Rule 2 on running_mean / running_var / num_batches_tracked after the steps ``inps`` (in order)."""
    C = inps[0].C
    rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    bm, bv = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
    for i, inp in enumerate(inps):
        st = inp.st
        m = 1.0 / (i + 1) if momentum is None else momentum
        unb = st.var * st.M / (st.M - 1)
        dmean, dvar, _ = stat_bounds(inp, D)
        bm = (1 - m) * bm + m * dmean + 3 * U24 * ((1 - m) * rm.abs() + m * st.mean.abs())
        bv = (1 - m) * bv + m * dvar * st.M / (st.M - 1) + 3 * U24 * ((1 - m) * rv.abs() + m * unb)
        rm, rv = (1 - m) * rm + m * st.mean, (1 - m) * rv + m * unb
    _elem(t, case, "running_mean", "rule2", mod.running_mean.cpu(), rm, bm)
    _elem(t, case, "running_var", "rule2", mod.running_var.cpu(), rv, bv)
    t.true(case, "num_batches_tracked = %d" % int(mod.num_batches_tracked), int(mod.num_batches_tracked) == len(inps))


# --------------------------------------------------------------------------- runners

def make_bn(device, inp, v=VARIANTS["bn"], **kw):
    from gaussiank_sgd_amd.ops.bn import BNAct
    m = BNAct(inp.C, act="relu" if v.relu else None, twin=v.twin, affine=inp.affine, **kw).to(device)
    if inp.affine:
        with torch.no_grad():
            m.weight.copy_(inp.gamma)
            m.bias.copy_(inp.beta)
    return m.train()


def bn_run(device, inp, v, mod=None, single=False):
    """One training step of BNAct; ``single``: a twin variant run as ONE output with the gradient dy + dy2."""
    twin = v.twin and not single
    m = mod if mod is not None else make_bn(device, inp, v._replace(twin=twin))
    x = rc._leaf(inp.x, device)
    res = rc._leaf(inp.res, device) if v.res else None
    assert x.is_contiguous(memory_format=CL) and m.fused_ok(x) == is_gpu(device)
    out = m(x, res)
    dy, dy2 = inp.dy.to(device), inp.dy2.to(device)
    if twin:
        y = out[0]
        assert out[1].data_ptr() == y.data_ptr()
        torch.autograd.backward([out[0], out[1]], [dy, dy2])
    else:
        y = out
        y.backward(dy + dy2 if v.twin else dy)
    return dict(y=y.detach(), dx=x.grad, dres=res.grad if v.res else None,
                dg=m.weight.grad if inp.affine else None, db=m.bias.grad if inp.affine else None, mod=m)


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in ("y", "dx", "dres", "dg", "db"))


# --------------------------------------------------------------------------- scenarios shared by CPU and GPU

def scenario_geometry(device, name, cd, D):
    """G: the five variants of one geometry case at the current number of workgroups."""
    t = Tally("G %s %s" % (name, cdname(cd)))
    inp = bn_inputs(g_shape(name, cd), cd)
    assert inp.offset == (name in ("m2", "m3")), float(kappa(inp.st).max())     # every other case: the yardstick
    for vn, v in VARIANTS.items():
        ours = bn_run(device, inp, v)
        bn_check(t, vn, ours, inp, v, D, is_gpu(device))
        running_check(t, vn, ours["mod"], [inp], D)
        if v.twin:
            t.true(vn, "twin differs from the single gradient dy + dy2",
                   same_bits(ours, bn_run(device, inp, v, single=True)))
        if vn == "res_relu":
            t.true(vn, "two runs differ", same_bits(ours, bn_run(device, inp, v)))
    t.finish()


def scenario_semantics(device, cd, D):
    """S: mixed-sign gamma, affine=False, momentum=None, three steps of running statistics."""
    t = Tally("S semantics " + cdname(cd))
    shape = S_SHAPE[cd]
    inp = bn_inputs(shape, cd, gamma="mixed")
    assert {float(s) for s in inp.gamma.sign()} == {-1.0, 0.0, 1.0} and not inp.offset
    for vn in ("relu", "res_relu", "twin_res"):
        bn_check(t, "gamma-mixed " + vn, bn_run(device, inp, VARIANTS[vn]), inp, VARIANTS[vn], D, is_gpu(device))
    # one constant channel among normal ones: its variance is exactly 0 (the one offset channel of the case),
    # the others stay on the yardstick
    cc = bn_inputs(shape, cd, const=2, seed=4)
    assert cc.off.tolist() == [float(c == 2) for c in range(cc.C)] and float(cc.st.var[2]) == 0.0
    for vn in ("bn", "res_relu"):
        ours = bn_run(device, cc, VARIANTS[vn])
        bn_check(t, "constant channel " + vn, ours, cc, VARIANTS[vn], D, is_gpu(device))
        running_check(t, "constant channel " + vn, ours["mod"], [cc], D)
    na = bn_inputs(shape, cd, affine=False)
    ours = bn_run(device, na, VARIANTS["res_relu"])
    bn_check(t, "affine=False", ours, na, VARIANTS["res_relu"], D, is_gpu(device))
    running_check(t, "affine=False", ours["mod"], [na], D)
    steps = [bn_inputs(shape, cd, mean=m, seed=i) for i, m in enumerate((0.0, 1.0, -2.0))]
    for momentum, n in ((None, 2), (MOM, 3)):
        mod = make_bn(device, steps[0], momentum=momentum)
        for inp_i in steps[:n]:
            bn_run(device, inp_i, VARIANTS["bn"], mod=mod)
        running_check(t, "momentum=%s x%d" % (momentum, n), mod, steps[:n], D, momentum)
    t.finish()


def scenario_single_value(device):
    """One value per channel (M = 1), and none: training-mode BatchNorm raises; the fused path must too."""
    def outcome(m, x):
        try:
            y = m(x)
        except Exception as e:                      # noqa: BLE001
            y = type(e).__name__ + ": " + str(e)
        return y, m.running_mean.cpu(), m.running_var.cpu(), int(m.num_batches_tracked)

    for shape in ((1, 64, 1, 1), (0, 64, 2, 2)):
        for cd in (F32, BF16):
            x = torch.ones(shape, dtype=cd, device=device).contiguous(memory_format=CL)
            assert x.numel() // 64 <= 1
            ours = outcome(make_bn(device, SimpleNamespace(C=64, affine=True, gamma=torch.ones(64),
                                                           beta=torch.zeros(64))), x)
            ref = outcome(torch.nn.BatchNorm2d(64).to(device).train(), x)
            if shape[0] == 1:
                assert isinstance(ref[0], str) and ref[0].startswith("ValueError: Expected more than 1 value per channel")
            assert type(ours[0]) is type(ref[0]), (shape, cd, ours[0], ref[0])
            if isinstance(ref[0], str):
                assert ours[0] == ref[0]
            else:
                assert ours[0].shape == ref[0].shape and ours[0].dtype == ref[0].dtype
            assert torch.equal(ours[1], ref[1]) and torch.equal(ours[2], ref[2]) and ours[3] == ref[3]
            assert not torch.isnan(ours[2]).any()


# --------------------------------------------------------------------------- P. BN + ReLU + max-pool

@functools.lru_cache(maxsize=None)
def pool_grads(shape, cd, pool):
    N, C, H, W = shape
    OH, OW = pool_out(H, W, pool)
    gen = torch.Generator().manual_seed(977 * pool[0] + 31 * pool[1] + pool[2] + C)
    oshape = (N, C, OH, OW)
    return nchw(_grid(gen, N * OH * OW, C, cd), oshape), nchw(_grid(gen, N * OH * OW, C, cd), oshape)


def _taps(zn, pool, fill):
    """The k * k strided slices of the padded plane, in the kernel's scan order, with their pixel indices."""
    k, s, p = pool
    N, C, H, W = zn.shape
    OH, OW = pool_out(H, W, pool)
    zp = F.pad(zn, (p, p, p, p), value=fill)
    oh = torch.arange(OH).view(OH, 1) * s - p
    ow = torch.arange(OW).view(1, OW) * s - p
    for kh in range(k):
        for kw in range(k):
            yield zp[:, :, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s], (oh + kh) * W + (ow + kw)


def _bf16_midpoint_dist(z):
    """Distance of fp64 z to the nearest midpoint between two bf16 values (where its rounding flips)."""
    zr = z.to(BF16)
    bits = zr.abs().view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(BF16).double()
    dn = (bits - 1).clamp(min=0).to(torch.int16).view(BF16).double()
    a, m = z.abs(), zr.abs().double()
    return torch.minimum((a - (m + up) / 2).abs(), (a - (m + dn) / 2).abs())


def pool_decide(zn, pool, cd, E, exact=None):
    """fp64 decisions of relu + max-pool on z ([N, C, H, W]; bf16: on the bf16-rounded z): the first maximum
    of each window as a pixel index, whether the ReLU blocks it, and whether the window is decided (rule 5)."""
    v = zn.to(BF16).double() if cd == BF16 else zn
    m1 = m2 = idx = None
    for tap, pix in _taps(v, pool, -math.inf):
        if m1 is None:
            m1, m2, idx = tap.clone(), torch.full_like(tap, -math.inf), pix.expand_as(tap).clone()
            continue
        upd = tap > m1
        m2 = torch.where(upd, m1, torch.maximum(m2, tap))
        idx = torch.where(upd, pix.expand_as(tap), idx)
        m1 = torch.where(upd, tap, m1)
    if cd == BF16:
        unsafe = (_bf16_midpoint_dist(zn) <= E).double()
        bad = torch.zeros_like(m1, dtype=torch.bool)
        for (tap, _), (uns, _) in zip(_taps(v, pool, -math.inf), _taps(unsafe, pool, 0.0)):
            bad |= (tap >= m1 - 2.0 ** -6 * m1.abs()) & (uns > 0)
        decided = ~bad & (m1.abs() > E)
    else:
        decided = (m1 - m2 > E) & (m1.abs() > E)
    if exact is not None:
        # gamma == 0: z = fma(x, 0, beta) is beta in any arithmetic, every window an exact tie (first tap wins)
        decided = torch.where(exact.view(1, -1, 1, 1), m1.abs() > E, decided)
    return idx, ~(m1 > 0), decided


def pool_ref(inp, pool, twin, idx, blocked):
    """fp64 BN + ReLU + max-pool forward and backward with the given decisions ([N, C, OH, OW])."""
    N, C, H, W = inp.shape
    st, g, b = inp.st, inp.gamma.double(), inp.beta.double()
    z = st.xhat * g + b
    zn = nchw(z, inp.shape).contiguous()
    flat = idx.reshape(N, C, -1)
    y = torch.where(blocked, torch.zeros((), dtype=F64), zn.reshape(N, C, H * W).gather(2, flat).view_as(idx))
    dy, dy2 = pool_grads(inp.shape, inp.cd, pool)
    dyt = dy.double() + (dy2.double() if twin else 0.0)
    dzn = torch.zeros(N, C, H * W, dtype=F64).scatter_add_(
        2, flat, torch.where(blocked, torch.zeros((), dtype=F64), dyt).reshape(N, C, -1)).view(N, C, H, W)
    r = _bn_backward(inp, dict(y=y, zn=zn, dz=rows(dzn)))
    return r


def pool_torch(inp, pool, twin, dt=F32):
    """bn -> relu -> max_pool2d of PyTorch on the CPU at ``dt`` with its own decisions."""
    x = inp.x.to(dt).clone().requires_grad_(True)
    w, b = inp.gamma.clone().requires_grad_(True), inp.beta.clone().requires_grad_(True)
    y, idx = F.max_pool2d(F.relu(F.batch_norm(x, None, None, w, b, True, 0.0, EPS)), *pool, return_indices=True)
    dy, dy2 = pool_grads(inp.shape, inp.cd, pool)
    y.backward((dy.to(dt) + dy2.to(dt)) if twin else dy.to(dt))
    return dict(y=y.detach(), dx=x.grad, dg=w.grad, db=b.grad, idx=idx, blocked=~(y.detach() > 0))


def pool_run_module(device, inp, pool, twin, single=False):
    """BNAct(pool=...) on ``device`` (the fallback on the CPU); the decisions are those of the same composition."""
    from gaussiank_sgd_amd.ops.bn import BNAct
    tw = twin and not single
    m = BNAct(inp.C, act="relu", pool=pool, twin=tw).to(device).train()
    with torch.no_grad():
        m.weight.copy_(inp.gamma)
        m.bias.copy_(inp.beta)
    x = rc._leaf(inp.x, device)
    out = m(x)
    dy, dy2 = (g.to(device) for g in pool_grads(inp.shape, inp.cd, pool))
    if tw:
        torch.autograd.backward([out[0], out[1]], [dy, dy2])
        y = out[0].detach()
    else:
        out.backward(dy + dy2 if twin else dy)
        y = out.detach()
    return dict(y=y, dx=x.grad, dg=m.weight.grad, db=m.bias.grad, mod=m)


def amax_decisions(amax, inp, pool):
    """The argmax bytes of bn_relu_pool_forward ([N, OH, OW, C]) as pixel indices and blocked flags
    ([N, C, OH, OW]); (ok, ...): every unblocked byte names a tap inside the image."""
    k, s, p = pool
    N, C, H, W = inp.shape
    OH, OW = pool_out(H, W, pool)
    a = amax.cpu().view(N, OH, OW, C).permute(0, 3, 1, 2).long()
    blocked = a == 255
    kh, kw = a // k, a % k
    ih = torch.arange(OH).view(1, 1, OH, 1) * s - p + kh
    iw = torch.arange(OW).view(1, 1, 1, OW) * s - p + kw
    ok = blocked | ((a < k * k) & (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W))
    idx = torch.where(blocked | ~ok, torch.zeros_like(a), ih * W + iw)
    return bool(ok.all()), idx, blocked


def pool_run_raw(device, inp, pool, twin):
    """bn_relu_pool_forward / bn_relu_pool_backward called directly (they expose the argmax bytes)."""
    ops = torch.ops.gksgd
    k, s, p = pool
    N, C, H, W = inp.shape
    OH, OW = pool_out(H, W, pool)
    x = inp.x.to(device)
    assert x.is_contiguous(memory_format=CL)
    y = torch.empty((N, C, OH, OW), dtype=inp.cd, device=device).contiguous(memory_format=CL)
    amax = torch.full((N * C * OH * OW,), 77, dtype=torch.uint8, device=device)
    stt = torch.full((4, C), math.nan, device=device)
    ws = torch.full((int(ops.bn_workspace_floats(inp.M, C, ebytes(inp.cd))),), math.nan, device=device)
    rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
    nbt = torch.zeros(1, dtype=torch.long, device=device)
    w, b = inp.gamma.to(device), inp.beta.to(device)
    ops.bn_relu_pool_forward(x, y, amax, w, b, rm, rv, stt[0], stt[1], stt[2], stt[3], ws, EPS, MOM, k, s, p, nbt,
                             None, 0)
    dy, dy2 = (g.to(device) for g in pool_grads(inp.shape, inp.cd, pool))
    dx = torch.full_like(x, math.nan)            # every pixel must be written, the uncovered ones too
    assert dx.is_contiguous(memory_format=CL)
    g = torch.full((2, C), math.nan, device=device)
    ops.bn_relu_pool_backward(dy, amax, x, dx, w, stt[0], stt[1], g[0], g[1], ws, k, s, p, None, None,
                              dy2 if twin else None)
    return dict(y=y, dx=dx, dg=g[0], db=g[1], amax=amax, mean=stt[0], invstd=stt[1], nbt=nbt)


def pool_check(t, case, ours, decisions, inp, pool, twin, D, Dp):
    """Rules 3-5 for one pool run; ``D``: depth of the statistics pass, ``Dp``: of the backward reduction."""
    idx, blocked = decisions
    r = pool_ref(inp, pool, twin, idx, blocked)
    yd = pool_torch(inp, pool, twin)
    ry = pool_ref(inp, pool, twin, yd["idx"], yd["blocked"])
    # E: the yardstick of the full-resolution z would be the natural margin; the pooled y is a subset of it
    Ey, Edx = FACTOR * _maxerr(yd["y"], ry["y"]), FACTOR * _maxerr(rows(yd["dx"]), ry["dx"])
    i64, b64, decided = pool_decide(r["zn"], pool, inp.cd, Ey, exact=inp.gamma == 0)
    same = (blocked == b64) & (blocked | (idx == i64))
    _undecided(t, case, "pool argmax", decided, same)
    dmean, dvar, rel_is = stat_bounds(inp, D)
    b_db, b_dg, _ = grad_bounds(inp, r, Dp, dmean, rel_is)
    by, bdx = torch.full_like(r["y"], Ey), torch.full_like(r["dx"], Edx)
    rule = "yardstick"
    if inp.cd == BF16:
        by, bdx, rule = BF16_ULP * r["y"].abs() + by, BF16_ULP * r["dx"].abs() + bdx, "bf16-out"
    t.true(case, "NaN / unwritten pixels in dx", not torch.isnan(ours["dx"]).any())
    _elem(t, case, "y", rule, ours["y"].cpu(), r["y"], by)
    _elem(t, case, "dx", rule, rows(ours["dx"]), r["dx"], bdx)
    _elem(t, case, "dbeta", "fp32-sum", ours["db"].cpu(), r["db"], b_db)
    _elem(t, case, "dgamma", "fp32-sum+rule2", ours["dg"].cpu(), r["dg"], b_dg)


def pool_depths(inp, pool, blocks):
    """(depth of the statistics pass at ``blocks``, depth of the pool backward's reduction)."""
    eb = ebytes(inp.cd)
    D = depth(bn_geo(inp.M, inp.C, eb, blocks))
    if pool_path(pool) == "tile" and pool_tiles(inp.shape, pool) <= inp.M:
        g = bn_geo(pool_tiles(inp.shape, pool), inp.C, eb, POOL_BLOCKS)
        return D, 4 * (-(-g.rpb // g.rl)) + 1               # a tile adds its four pixels
    return D, depth(bn_geo(inp.M, inp.C, eb, POOL_BLOCKS))


def scenario_pool(device, cd, path, shape=None, pools=None, blocks=None, twins=(False, True)):
    """P: every pool of one backward path, twin off and on, mixed-sign gamma (``blocks``: the workgroups of
    the statistics pass; the pool backward sizes its own grid)."""
    t = Tally("P pool %s %s" % (path, cdname(cd)))
    inp = bn_inputs(shape or P_SHAPE[cd], cd, gamma="mixed", seed=3)
    assert not inp.offset
    for pool in (pools or P_POOLS[path]):
        for twin in twins:
            case = "k%d s%d p%d%s" % (pool + (" twin" if twin else "",))
            D, Dp = pool_depths(inp, pool, blocks or default_blocks())
            if is_gpu(device):
                ours = pool_run_raw(device, inp, pool, twin)
                ok, idx, blocked = amax_decisions(ours["amax"], inp, pool)
                t.true(case, "an argmax byte names a tap outside the window or the image", ok)
                mod = pool_run_module(device, inp, pool, twin)
                t.true(case, "BNAct(pool) differs from the raw ops",
                       all(torch.equal(mod[k_], ours[k_]) for k_ in ("y", "dx", "dg", "db")))
                if twin:
                    one = pool_run_module(device, inp, pool, twin, single=True)
                    t.true(case, "twin differs from the single gradient dy + dy2",
                           all(torch.equal(mod[k_], one[k_]) for k_ in ("y", "dx", "dg", "db")))
            else:
                ours = pool_run_module(device, inp, pool, twin)
                yd = pool_torch(inp, pool, twin, dt=cd)
                idx, blocked = yd["idx"], yd["blocked"]
            pool_check(t, case, ours, (idx, blocked), inp, pool, twin, D, Dp)
    t.finish()


# --------------------------------------------------------------------------- N. statistics envelope

def scenario_envelope(device, cd, mean, std, blocks, extra=None):
    """N: one-pass variance at (mean, std) on the multi-row shape; ``extra(t, case, inp)``: the raw-op checks
    of the GPU test.  std 1: rule 2's invstd bound must be <= 1e-2, asserted from the reference."""
    t = Tally("N envelope " + cdname(cd))
    case = "mean %g std %g" % (mean, std)
    inp = bn_inputs(N_SHAPE, cd, mean=mean, std=std)
    assert inp.offset == (mean != 0.0)
    D = depth(bn_geo(inp.M, inp.C, ebytes(cd), blocks))
    _, _, rel_is = stat_bounds(inp, D)
    print("ENV | %s | %s | D %d | rule-2 relative invstd bound %.3e | (mean / std)^2 %.3g" % (
        t.family, case, D, float(rel_is.max()), float((inp.st.mean ** 2 / inp.st.var.clamp(min=1e-30)).max())))
    if std == 1.0:
        assert float(rel_is.max()) <= 1e-2, float(rel_is.max())
    ours = bn_run(device, inp, VARIANTS["relu"])
    bn_check(t, case, ours, inp, VARIANTS["relu"], D, is_gpu(device))
    running_check(t, case, ours["mod"], [inp], D)
    if extra is not None:
        extra(t, case, inp)
    t.finish()


# --------------------------------------------------------------------------- constant channels

@functools.lru_cache(maxsize=None)
def constant_inputs(cd):
    """Every channel constant, at values whose squares do not add exactly into the fp32 partial of a block of
    281 rows (bf16 values have 8 significant bits, so the shape must be the long one): q / M - mean^2 comes
    out a little above or below 0, and below 0 only the clamp keeps var + eps positive."""
    base = bn_inputs(g_shape("minc_rows", cd), cd, seed=9)
    inp = SimpleNamespace(**vars(base))
    vals = (torch.tensor([255.0 - 2 * c for c in range(inp.C)]) if cd == BF16
            else torch.tensor([300.3 + 0.7 * c for c in range(inp.C)]))
    xr = vals.to(cd).expand(inp.M, inp.C).contiguous()
    v64 = vals.to(cd).double()
    inp.st = SimpleNamespace(M=inp.M, mean=v64, var=torch.zeros_like(v64), invstd=torch.full_like(v64, EPS ** -0.5),
                             xhat=torch.zeros(inp.M, inp.C, dtype=F64), absmean=v64.abs(), sqmean=v64 * v64)
    inp.x, inp.offset, inp.off = nchw(xr, inp.shape), True, torch.ones(inp.C, dtype=F64)
    return inp


def scenario_constant(device, cd, D, extra=None):
    """var = 0 exactly: invstd must stay within [1 / sqrt(|d var| + eps), 1 / sqrt(eps)] (the ``var < 0`` clamp;
    ``extra`` of the GPU test checks save_invstd), y = beta up to the cancellation of x scale + shift.
    ``D``: the depth of rule 2 (the kernel's geometry on the GPU)."""
    t = Tally("S constant " + cdname(cd))
    inp = constant_inputs(cd)
    st, g = inp.st, inp.gamma.double()
    dmean, dvar, _ = stat_bounds(inp, D)
    ours = bn_run(device, inp, VARIANTS["bn"])
    y, dx = rows(ours["y"]), rows(ours["dx"])
    t.true("const", "NaN / inf in y or dx", bool(torch.isfinite(y).all() and torch.isfinite(dx).all()))
    # y = fma(x, sc, sf), sc = fl(g is), sf = fl(beta - fl(fl(mean g) is)), is <= 1 / sqrt(eps)
    by = g.abs() / math.sqrt(EPS) * (dmean + 4 * U24 * st.absmean) * (1 + 2 * U24) + 2 * U24 * inp.beta.double().abs()
    if cd == BF16:
        by = by + BF16_ULP * (inp.beta.double().abs() + by)
    _elem(t, "const", "y", "derived", y, inp.beta.double().expand_as(y), by)
    dz = rows(inp.dy)
    _elem(t, "const", "dbeta", "fp32-sum", ours["db"].cpu(), dz.sum(0), D * FP32_SUM * dz.abs().sum(0) +
          U24 * dz.sum(0).abs())
    running_check(t, "const", ours["mod"], [inp], D)
    rv = ours["mod"].running_var.cpu().double()
    t.true("const", "running_var below (1 - momentum): a negative variance got through",
           bool((rv >= (1 - MOM) * (1 - 4 * U24)).all()))
    if extra is not None:
        extra(t, "const", inp, dvar)
    t.finish()


# --------------------------------------------------------------------------- raw ops (GPU only)

def raw_partials(device, inp, blocks):
    """bn_stats_partials at the current number of workgroups -> (geometry, [2, gy, C] partials on the CPU)."""
    ops = torch.ops.gksgd
    g = bn_geo(inp.M, inp.C, ebytes(inp.cd), blocks)
    ws = torch.full((int(ops.bn_workspace_floats(inp.M, inp.C, ebytes(inp.cd))),), math.nan, device=device)
    assert ws.numel() >= 2 * g.gy * inp.C
    ops.bn_stats_partials(inp.x.to(device), ws)
    assert bool(torch.isnan(ws[2 * g.gy * inp.C:]).all()), "the pass wrote past the 2 gy C partials of %d workgroups" % blocks
    return g, ws[:2 * g.gy * inp.C].view(2, g.gy, inp.C).cpu()


def block_sums(xr, edges):
    """fp64 per-block sums of the rows [edges[i], edges[i + 1]) -> [blocks, C]."""
    return torch.stack([xr[a:b].sum(0) if b > a else torch.zeros(xr.shape[1], dtype=F64)
                        for a, b in zip(edges[:-1], edges[1:])])


def partials_check(t, case, inp, g, part):
    """Rule 1."""
    xr = rows(inp.x)
    br = block_rows(g)
    edges = [min(g.M, b * g.rpb) for b in range(g.gy + 1)]
    n = torch.tensor([float(depth(g, r)) for r in br]).view(-1, 1)
    t.fp32_sum(case, "psum", part[0], block_sums(xr, edges), n, block_sums(xr.abs(), edges))
    t.fp32_sum(case, "psq", part[1], block_sums(xr * xr, edges), n, block_sums(xr * xr, edges))
    for b, r in enumerate(br):
        if r == 0:
            t.true(case, "empty workgroup %d must write exact zeros" % b, not part[:, b].any())


def raw_finalize(device, inp, pre=None, pre_rows=0):
    """bn_act_finalize (statistics pass + finalize, or the finalize of given partials)."""
    ops = torch.ops.gksgd
    C = inp.C
    stt = torch.full((4, C), math.nan, device=device)
    ws = torch.full((int(ops.bn_workspace_floats(inp.M, C, ebytes(inp.cd))),), math.nan, device=device)
    rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
    nbt = torch.zeros(1, dtype=torch.long, device=device)
    w, b = (inp.gamma.to(device), inp.beta.to(device)) if inp.affine else (None, None)
    ops.bn_act_finalize(inp.x.to(device), w, b, rm, rv, stt[0], stt[1], stt[2], stt[3], ws, EPS, MOM, nbt, pre, pre_rows)
    return SimpleNamespace(mean=stt[0].cpu(), invstd=stt[1].cpu(), scale=stt[2].cpu(), shift=stt[3].cpu(),
                           running_mean=rm, running_var=rv, num_batches_tracked=nbt)


def finalize_check(t, case, inp, out, D):
    """Rule 2 on save_mean / save_invstd and the running statistics of one raw finalize."""
    dmean, dvar, rel_is = stat_bounds(inp, D)
    _elem(t, case, "save_mean", "rule2", out.mean, inp.st.mean, dmean)
    _elem(t, case, "save_invstd", "rule2", out.invstd, inp.st.invstd, rel_is * inp.st.invstd)
    running_check(t, case, out, [inp], D)


def uneven_edges(M):
    """Five uneven blocks of rows, one of a single row."""
    return [0, 1, M // 3, M // 3 + 7, M - 2, M] if M >= 16 else [0, 1, 1, M - 1, M - 1, M]


def pre_partials(device, cols, edges, alloc=9):
    """fp32 [2, alloc, C] partials from fp64 block sums of the two column sets; NaN in the rows past the blocks."""
    nb = len(edges) - 1
    part = torch.full((2, alloc, cols[0].shape[1]), math.nan)
    part[0, :nb], part[1, :nb] = block_sums(cols[0], edges).float(), block_sums(cols[1], edges).float()
    return part.to(device), nb


def scenario_forward_pre(device, cd):
    """``pre`` partials with pre_rows < part.size(1): bn_act_forward and bn_act_finalize must read the first
    pre_rows rows only (NaN behind them).  The partials are exact block sums rounded to fp32: rule 2 at D = 1."""
    ops = torch.ops.gksgd
    t = Tally("S pre " + cdname(cd))
    for name in ("idle", "multirow"):
        inp = bn_inputs(g_shape(name, cd), cd, seed=5)
        xr = rows(inp.x)
        pre, nb = pre_partials(device, (xr, xr * xr), uneven_edges(inp.M))
        assert nb < pre.shape[1]
        finalize_check(t, name + " finalize", inp, raw_finalize(device, inp, pre, nb), 1)
        for relu in (False, True):
            x = inp.x.to(device)
            y = torch.full_like(x, math.nan)
            C, eb = inp.C, ebytes(cd)
            mask = torch.zeros(int(ops.bn_mask_bytes(inp.M, C, eb)), dtype=torch.uint8, device=device) if relu else None
            stt = torch.full((4, C), math.nan, device=device)
            ws = torch.full((int(ops.bn_workspace_floats(inp.M, C, eb)),), math.nan, device=device)
            out = SimpleNamespace(running_mean=torch.zeros(C, device=device), running_var=torch.ones(C, device=device),
                                  num_batches_tracked=torch.zeros(1, dtype=torch.long, device=device))
            ops.bn_act_forward(x, None, y, mask, inp.gamma.to(device), inp.beta.to(device), out.running_mean,
                               out.running_var, stt[0], stt[1], stt[2], stt[3], ws, EPS, MOM, relu,
                               out.num_batches_tracked, pre, nb)
            case = "%s forward relu=%d" % (name, relu)
            out.mean, out.invstd = stt[0].cpu(), stt[1].cpu()
            finalize_check(t, case, inp, out, 1)
            bn_check(t, case, dict(y=y), inp, VARIANTS["relu" if relu else "bn"], 1, True, fwd_only=True)
    t.finish()


def scenario_backward_pre(device, cd, mean):
    """bn_act_backward_pre: finalize of given sum(dz), sum(dz x) partials (the ``cmean`` branch) + apply.
    The fp32 partials, mean and invstd are inputs as stored, so the reference takes them as they are:
    dbeta and dgamma = invstd (sum(dz x) - mean sum(dz)) are then one fp32 rounding of an fp64 result."""
    ops = torch.ops.gksgd
    t = Tally("S backward_pre " + cdname(cd))
    inp = bn_inputs(N_SHAPE, cd, mean=mean, seed=6)
    case = "mean %g" % mean
    xr, dz = rows(inp.x), rows(inp.dy)
    part, nb = pre_partials(device, (dz, dz * xr), uneven_edges(inp.M))
    mu32, is32 = inp.st.mean.float(), inp.st.invstd.float()
    x, dzt = inp.x.to(device), inp.dy.to(device)
    dx = torch.full_like(x, math.nan)
    g = torch.full((2, inp.C), math.nan, device=device)
    w = inp.gamma.to(device)
    ops.bn_act_backward_pre(dzt, x, dx, w, mu32.to(device), is32.to(device), g[0], g[1], part, nb, None, None, None)
    p = part.cpu()[:, :nb].double()
    mu, istd, gam = mu32.double(), is32.double(), inp.gamma.double()
    db = p[0].sum(0)
    dg = istd * (p[1].sum(0) - mu * db)
    xhat = (xr - mu) * istd
    ref = gam * istd * (dz - db / inp.M - xhat * dg / inp.M)
    _elem(t, case, "dbeta", "one rounding", g[1].cpu(), db, FP32_SUM * db.abs())
    # fp64 cancellation of sum(dz x) - mean sum(dz): 2^-52 of the operands
    _elem(t, case, "dgamma", "one rounding", g[0].cpu(), dg, FP32_SUM * dg.abs() + 2.0 ** -50 * istd * (
        p[1].abs().sum(0) + mu.abs() * p[0].abs().sum(0)))
    x32 = inp.x.float().contiguous(memory_format=CL)
    yard = torch.ops.aten.native_batch_norm_backward(inp.dy.float(), x32, inp.gamma, None, None, mu32, is32, True, EPS,
                                                     [True, False, False])[0]
    # the yardstick reduces sum(dz) and sum(dz xhat) itself; its reference is the fp64 backward of the same dz
    dby, dgy = dz.sum(0), (dz * xhat).sum(0)
    E = FACTOR * _maxerr(rows(yard), gam * istd * (dz - dby / inp.M - xhat * dgy / inp.M))
    bdx = torch.full_like(ref, E)
    if cd == BF16:
        bdx = BF16_ULP * ref.abs() + bdx
    t.true(case, "NaN in dx", not torch.isnan(dx).any())
    _elem(t, case, "dx", "bf16-out" if cd == BF16 else "yardstick", rows(dx), ref, bdx)
    t.finish()
