"""Shared cases of the BERT row-kernel tests: fused add + dropout + LayerNorm
(ln.hip), softmax cross-entropy (xent.hip), the input embedding (embed.hip) and
the GELU backward + bias column sum (linear.hip).  tests/test_bert_rows_cpu.py
runs them through the pure-PyTorch fallbacks of ``ops.ln.add_layernorm``,
``ops.xent.cross_entropy``, ``ops.embedding.bert_embeddings`` and
``ops.linear.gelu_backward_``; tests/test_bert_rows_gpu.py runs the same cases
on the HIP kernels.  Every runner takes the device; every reference is fp64
PyTorch on the CPU, on the inputs as stored (bf16 inputs are the bf16 values
cast to fp64), computed once per case and shared (``functools.lru_cache``).

Tolerance rules
---------------
Four rules; no rule looks at the output of the code under test to size itself.

1. bf16-stored output (``Tally.bf16_out``): elementwise
   ``|ours - ref| <= 2^-8 |ref| + E``.  bf16 has 8 significand bits: in
   [2^k, 2^(k+1)) its values are 2^(k-7) apart, so round-to-nearest-even moves
   a value v by at most 2^(k-8) <= 2^-8 |v|, with equality just above a power
   of two (the measured ratios reach 0.996).  ``E`` covers the fp32 math before
   the rounding and is ``FACTOR`` times the max-abs error of PyTorch's own
   fp32 implementation of the op against fp64 on the same case (rule 3).

2. fp32 sum of ``n`` terms (``Tally.fp32_sum``): elementwise
   ``|ours - ref| <= n 2^-23 sum|terms|``.  Any summation order of n fp32
   terms has error <= gamma_(n-1) sum|terms| with gamma_k = k u / (1 - k u),
   u = 2^-24; n 2^-23 is twice gamma_n to first order.  The terms must be exact
   in fp32 (stored gradients), so the rule is used for dbeta (column sums of
   dy), the embedding tables (sums of dy rows; n = the id's token count, the
   batch size, the type's token count) and the GELU bias gradient (column
   sums of dpre as stored).  A value that is accumulated onto a stored fp32
   ``init`` (direct-arena LayerNorm) counts ``init`` as one more term.

3. the yardstick (``Tally.yard``), where no bound can be derived: PyTorch's own
   implementation of the op (``F.layer_norm``, ``F.cross_entropy``,
   ``aten.gelu_backward``) at the kernel's precision -- fp32 tensors for fp32
   storage, bf16 tensors for bf16 storage -- on the same inputs; its max-abs
   error against fp64, per output tensor, is the yardstick and ours must be
   <= ``FACTOR`` (= ``adam_cases.FACTOR`` = 2) times it (room for FMA
   contraction, ``__expf`` and operation order).  Used for the fp32-math term
   ``E`` of rule 1, for y / dx / da / dgamma of fp32-storage LayerNorm, for
   dx / da / dgamma of bf16-storage LayerNorm (they go through the bf16-stored
   ``h = x + drop(a)``, as PyTorch's bf16 composition does) and for the fp32
   GELU backward.

4. dgamma of ONE row on the fp32 kernels (``ln_dgamma_single_row_bound``).  With R = 1, dgamma[i] is the
   single product dy[i] * xhat[i]: nothing is summed, so the yardstick of a case is the luck of one product.
   In fp32 ulps of the largest element PyTorch's CPU layer_norm is off by 0.4 .. 2.2 over the fourteen A1
   row lengths and the kernels by 0.1 .. 2.3 -- the same class -- but where PyTorch happens to be correctly
   rounded (nc = 33: 0.46 ulp) twice its error is a one-ulp bound, which a 1-ulp ``rsqrtf`` and three more
   roundings cannot meet on every input (ours: 1.08 ulp, 2.35x; nc = 257: 2.02x).  The kernel is right
   there and PyTorch unusually exact, so the R = 1 cases of the fp32 kernels take a derived bound for dgamma
   and print the yardstick ratio without asserting it.
   With u = 2^-24, D = 8 CH + log2(64 / RPW) the longest chain of additions of a row sum (8 CH values per
   lane, then the butterfly), to first order:
     mean       |mu' - mu| <= delta = D u mean|h| + u |mu|        (sum of H terms, then one division)
     variance   sum of (h - mu')^2 (1 + 2u each: one subtraction, one fma) over a chain of D, / H, + eps:
                relative (D + 4) u, plus delta^2 rstd^2 for the shifted mean
     rstd       relative eps_rs = (D / 2 + 4) u + delta^2 rstd^2 / 2   (half of that, 1-ulp rsqrtf = 2u)
     xhat'      = fl(fl(h - mu') rstd'): |xhat' - xhat| <= |xhat| (eps_rs + 2u) + rstd delta
     dgamma     = fl(dy xhat'): |err| <= |dy| (|xhat| (eps_rs + 3u) + rstd delta), times 1.01 for the
                second-order terms; the partial-row reduction adds zeros and is exact.
   R = 19 and every other shape keep the yardstick for dgamma.

Every check prints ``TOL | family | case | tensor | rule | err | bound |
ratio``; profiles/bert_row_kernels_tolerances.txt is the worst line per family
and tensor of the GPU run.

Ignored rows (cross-entropy).  ``ops.xent.cross_entropy`` divides the summed
row losses by ``max(count, 1)`` where ``count`` is the number of labels that
differ from ``ignore_index``: an all-ignored batch gives loss 0.0 and an
all-zero gradient (``F.cross_entropy`` gives NaN there).  Labels outside
[0, V) contribute neither loss nor gradient but are still counted in the
divisor; the cases here use in-range labels only.
"""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

import adam_cases as ac

FACTOR = ac.FACTOR
BF16_ULP = 2.0 ** -8
FP32_SUM = 2.0 ** -23
EPS = 1e-5
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _cpu64(t):
    return t.detach().to("cpu", F64)


def _leaf(t, device="cpu", dt=None):
    """A fresh leaf on ``device``: the cached case tensors are shared and must never collect a gradient."""
    return t.detach().to(device, dt if dt is not None else t.dtype).clone().requires_grad_(True)


class Tally:
    """Collects the checks of one test; ``finish()`` fails with every miss listed."""

    def __init__(self, family):
        self.family = family
        self.fails = []

    def _rec(self, case, name, rule, err, bound, ratio, limit):
        print("TOL | %s | %s | %s | %s | err %.3e | bound %.3e | ratio %.3f" % (self.family, case, name, rule, err,
                                                                               bound, ratio))
        if not ratio <= limit:      # NaN fails
            self.fails.append("%s %s %s: err %.3e, %s bound %.3e, ratio %.3f (limit %g)" % (
                self.family, case, name, err, rule, bound, ratio, limit))

    @staticmethod
    def _ratio(d, bound):
        """max over elements of d / bound; an element with bound 0 must have d == 0."""
        if d.numel() == 0:
            return 0.0, 0.0, 0.0
        if torch.isnan(d).any():
            return float("nan"), float(bound.max()), float("nan")
        r = torch.where(bound > 0, d / bound.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, math.inf),
                                                                            torch.zeros_like(d)))
        i = int(r.argmax())
        return float(d.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(r.reshape(-1)[i])

    def yard(self, case, name, ours, ref, yard_t, enforce=True):
        """Rule 3: max|ours - ref| <= FACTOR * max|yard_t - ref| (``enforce=False``: printed only)."""
        ours, ref, yard_t = _cpu64(ours), _cpu64(ref), _cpu64(yard_t)
        assert ours.shape == ref.shape, (case, name, ours.shape, ref.shape)
        if ref.numel() == 0:
            return
        err = float((ours - ref).abs().max())
        y = float((yard_t - ref).abs().max())
        ratio = err / y if y > 0 else (0.0 if err == 0 else math.inf)
        self._rec(case, name, "yardstick" if enforce else "yardstick (not asserted)", err, y, ratio,
                  FACTOR if enforce else math.inf)

    def bf16_out(self, case, name, ours, ref, E):
        """Rule 1: elementwise |ours - ref| <= 2^-8 |ref| + E."""
        ours, ref = _cpu64(ours), _cpu64(ref)
        assert ours.shape == ref.shape, (case, name, ours.shape, ref.shape)
        self._rec(case, name, "bf16-out", *self._ratio((ours - ref).abs(), BF16_ULP * ref.abs() + E), 1.0)

    def fp32_sum(self, case, name, ours, ref, n, sumabs):
        """Rule 2: elementwise |ours - ref| <= n 2^-23 sum|terms| (n a number or a tensor that broadcasts)."""
        ours, ref = _cpu64(ours), _cpu64(ref)
        assert ours.shape == ref.shape, (case, name, ours.shape, ref.shape)
        bound = (torch.as_tensor(n, dtype=F64) * FP32_SUM * _cpu64(sumabs)).expand_as(ref)
        self._rec(case, name, "fp32-sum", *self._ratio((ours - ref).abs(), bound), 1.0)

    def true(self, case, what, cond):
        if not bool(cond):
            self.fails.append("%s %s: %s" % (self.family, case, what))

    def finish(self):
        assert not self.fails, "%d check(s) failed:\n%s" % (len(self.fails), "\n".join(self.fails))


def is_gpu(device):
    return torch.device(device).type == "cuda"


# --------------------------------------------------------------------------- A. add + dropout + LayerNorm

# ln_dispatch: (CH, RPW) from nc = H / 8 -- the thresholds of csrc/kernels/ln.hip written out
LN_BUCKETS = ((32, (1, 2)), (64, (2, 2)), (96, (3, 2)), (128, (4, 2)), (192, (6, 2)), (256, (8, 2)), (512, (8, 1)))
A1_NC = (1, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 512)
A1_R = (1, 19)            # odd, no multiple of the 16 rows of a backward block
LN_ROWS_PER_BLOCK = 16    # backward: one partial row per block
LN_FIN_SPLITS = 32        # kFinSplits


def ln_bucket(nc):
    for top, inst in LN_BUCKETS:
        if nc <= top:
            return inst
    raise ValueError(nc)


@functools.lru_cache(maxsize=None)
def ln_inputs(R, H, cd, offset=False):
    """a, x, dy in the storage dtype ``cd``; gamma, beta fp32 and non-trivial.  ``offset``: rows of
    h = x + a with mean 100 and standard deviation 0.1 (two-pass variance)."""
    gen = torch.Generator().manual_seed(1000 * R + H + (7 if cd == BF16 else 0) + (13 if offset else 0))
    if offset:
        x = 100.0 + 0.07 * torch.randn(R, H, generator=gen)
        a = 0.07 * torch.randn(R, H, generator=gen)
    else:
        x = torch.randn(R, H, generator=gen)
        a = torch.randn(R, H, generator=gen)
    return SimpleNamespace(R=R, H=H, cd=cd, a=a.to(cd), x=x.to(cd), dy=torch.randn(R, H, generator=gen).to(cd),
                           gamma=torch.rand(H, generator=gen) + 0.5, beta=torch.rand(H, generator=gen) - 0.5)


def ln_torch(inp, dt, mask=None, p=0.0):
    """PyTorch's LN(x + a * mask / (1 - p)) and its gradients with row tensors of dtype ``dt`` (fp64: the
    reference; fp32 / bf16: the yardstick).  gamma / beta stay fp32 below fp64, as the kernels keep them."""
    wdt = F64 if dt == F64 else F32
    a, x, g, b = _leaf(inp.a, dt=dt), _leaf(inp.x, dt=dt), _leaf(inp.gamma, dt=wdt), _leaf(inp.beta, dt=wdt)
    ad = a if mask is None else a * (mask.to(dt) * (1.0 / (1.0 - p)))
    y = F.layer_norm(x + ad, (inp.H,), g, b, EPS)
    y.backward(inp.dy.to(dt))
    return dict(y=y.detach(), dx=x.grad, da=a.grad, dg=g.grad, db=b.grad)


@functools.lru_cache(maxsize=None)
def ln_refs(R, H, cd, offset=False):
    inp = ln_inputs(R, H, cd, offset)
    return inp, ln_torch(inp, F64), ln_torch(inp, F32), (ln_torch(inp, BF16) if cd == BF16 else None)


def ln_dgamma_single_row_bound(inp):
    """Rule 4 (docstring of this module): the derived bound on the fp32 kernels' dgamma for R = 1."""
    assert inp.R == 1 and inp.cd == F32
    u = 2.0 ** -24
    ch, rpw = ln_bucket(inp.H // 8)
    D = 8 * ch + int(math.log2(64 // rpw))
    h = inp.x.double() + inp.a.double()
    mu = h.mean()
    rs = 1.0 / torch.sqrt(h.var(unbiased=False) + EPS)
    delta = D * u * h.abs().mean() + u * mu.abs()
    eps_rs = (D / 2 + 4) * u + 0.5 * (delta * rs) ** 2
    xhat = (h - mu) * rs
    return (inp.dy.double().abs() * (xhat.abs() * (eps_rs + 3 * u) + rs * delta))[0] * 1.01


def ln_check(tally, case, ours, inp, r64, r32, rbf, init=None, fused=True):
    """The LN rules: y bf16-out (bf16) or yardstick (fp32); dx, da, dgamma yardstick at the storage
    precision; dbeta the fp32 sum of R stored dy.  ``init`` = (dg0, db0): ours are accumulated onto them.
    ``fused=False``: ours is the PyTorch composition, which rounds h = x + a to bf16 BEFORE the LayerNorm
    (the kernel normalises the fp32 sum), so its bf16 y gets the bf16 yardstick instead of rule 1."""
    if inp.cd == BF16 and not fused:
        tally.yard(case, "y", ours["y"], r64["y"], rbf["y"])
        yd = rbf
    elif inp.cd == BF16:
        E = FACTOR * float((r32["y"].double() - r64["y"]).abs().max())
        tally.bf16_out(case, "y", ours["y"], r64["y"], E)
        yd = rbf
    else:
        tally.yard(case, "y", ours["y"], r64["y"], r32["y"])
        yd = r32
    for k in ("dx", "da"):
        tally.yard(case, k, ours[k], r64[k], yd[k])
    sumabs = inp.dy.double().abs().sum(0)
    if init is None:
        single = fused and inp.cd == F32 and inp.R == 1
        tally.yard(case, "dgamma", ours["dg"], r64["dg"], yd["dg"], enforce=not single)
        if single:
            bound = ln_dgamma_single_row_bound(inp)
            tally._rec(case, "dgamma", "single-row", *tally._ratio((_cpu64(ours["dg"]) - r64["dg"]).abs(), bound), 1.0)
        tally.fp32_sum(case, "dbeta", ours["db"], r64["db"], inp.R, sumabs)
    else:
        dg0, db0 = (_cpu64(t) for t in init)
        # ours = fp32(init + sum): the sum within the yardstick, then one fp32 add (2^-23 of the result)
        tot = dg0 + r64["dg"]
        err = float(((_cpu64(ours["dg"]) - tot).abs() - FP32_SUM * tot.abs()).clamp(min=0).max())
        y = float((yd["dg"].double() - r64["dg"]).abs().max())
        tally._rec(case, "dgamma(acc)", "yardstick", err, y, err / y if y > 0 else (0.0 if err == 0 else math.inf),
                   FACTOR)
        tally.fp32_sum(case, "dbeta(acc)", ours["db"], db0 + r64["db"], inp.R + 1, sumabs + db0.abs())


def ln_api(device, inp):
    """ops.ln.add_layernorm without dropout on ``device`` (the HIP kernels on a GPU, the composition elsewhere)."""
    from gaussiank_sgd_amd.ops.ln import add_layernorm
    ln = nn.LayerNorm(inp.H, eps=EPS).to(device)
    with torch.no_grad():
        ln.weight.copy_(inp.gamma)
        ln.bias.copy_(inp.beta)
    a, x = _leaf(inp.a, device), _leaf(inp.x, device)
    y = add_layernorm(a, x, ln, 0.0, True)
    y.backward(inp.dy.to(device))
    return dict(y=y.detach(), dx=x.grad, da=a.grad, dg=ln.weight.grad, db=ln.bias.grad)


def ln_fn(device, inp, p=0.0, seed=0, direct=None):
    """_AddLNFn.apply on the GPU with an explicit seed (seed_dev=None) and optional direct-arena views."""
    from gaussiank_sgd_amd.ops.ln import _AddLNFn
    a, x, g, b = _leaf(inp.a, device), _leaf(inp.x, device), _leaf(inp.gamma, device), _leaf(inp.beta, device)
    y = _AddLNFn.apply(a, x, g, b, EPS, p, seed, direct, None, inp.cd)
    y.backward(inp.dy.to(device))
    return dict(y=y.detach(), dx=x.grad, da=a.grad, dg=g.grad, db=b.grad)


def ln_fwd_mask(device, R, H, cd, p, seed):
    """Keep-mask recovered from the forward alone: a = 1, x = 0, gamma = 1, beta = 0 makes h = mask / (1 - p),
    so dropped elements lie below the row mean (y < 0) and kept ones above."""
    from gaussiank_sgd_amd.ops.ln import _AddLNFn
    one = torch.ones(R, H, dtype=cd, device=device)
    with torch.no_grad():
        y = _AddLNFn.apply(one, torch.zeros_like(one), torch.ones(H, device=device), torch.zeros(H, device=device),
                           EPS, p, seed, None, None, cd)
    return (y.float() > 0).cpu()


def ln_plain_masked(inp, mask, p):
    """Stand-in for the kernels off the GPU: PyTorch at the storage precision with a given mask."""
    a, x, g, b = _leaf(inp.a), _leaf(inp.x), _leaf(inp.gamma), _leaf(inp.beta)
    h = x + a * (mask.to(inp.cd) * (1.0 / (1.0 - p)))
    y = F.layer_norm(h.float(), (inp.H,), g, b, EPS).to(inp.cd)      # as the fallback of ops.ln.add_layernorm
    y.backward(inp.dy)
    return dict(y=y.detach(), dx=x.grad, da=a.grad, dg=g.grad, db=b.grad)


# --------------------------------------------------------------------------- B. softmax cross-entropy

XENT_V = (2, 6, 510, 512, 514, 1022, 1026, 30522)   # V / 2 below, at and above one and two 256-thread strides
XENT_R = 8
XENT_UP = 3.0                                        # (loss * 3).backward()
# (ignore_index, which rows are ignored): none; some; all but one; all
XENT_IGNORE = [(-100, "none"), (-100, "some"), (-100, "one-counted"), (-100, "all"),
               (0, "some"), (0, "one-counted"), (0, "all")]


@functools.lru_cache(maxsize=None)
def xent_rows(V):
    """Eight bf16 rows and labels in [0, V): every label position (0, V-1, an even and an odd index, both
    halves of the last pair) and every logit kind.  ``ninf``: the -inf positions of row 7."""
    gen = torch.Generator().manual_seed(V)
    even, odd = (V // 2) & ~1, ((V // 3) | 1) if V > 2 else 1
    labels = torch.tensor([0, V - 1, even, odd, V - 2, odd, even, V - 1])
    x = 30.0 * torch.randn(XENT_R, V, generator=gen)
    for r in (0, 1, 2, 3, 7):                        # label and pair neighbour near the row maximum: neither
        m = float(x[r].max())                        # softmax underflows, so both gradient signs are visible
        x[r, labels[r]], x[r, labels[r] ^ 1] = m - 2.0, m - 1.0
    x[4] = 1.25                                      # constant row: loss log V
    x[5] = torch.randn(V, generator=gen)
    x[5, labels[5]] = x[5].max() + 60.0              # confident: loss ~ 0, exp(x - lse) - 1 cancels
    x[6] = torch.randn(V, generator=gen)
    x[6, labels[6]] = x[6].min() - 60.0              # improbable label
    free = torch.tensor([v for v in range(V) if v != int(labels[7]) and v != (int(labels[7]) ^ 1)], dtype=torch.long)
    ninf = free[torch.randperm(len(free), generator=gen)[:(V - 1) // 4]]
    x[7, ninf] = -math.inf
    return x.to(BF16), labels, ninf


@functools.lru_cache(maxsize=None)
def xent_case(V, ignore, mode):
    logits, labels, ninf = xent_rows(V)
    labels = labels.clone()
    if mode != "none":
        # ignored rows carry ``ignore``; with ignore = 0 (a valid class id) a kept row whose label is 0 is
        # ignored as well (the rows kept below have odd labels for every V)
        keep = {"some": [1, 3, 5, 6, 7], "one-counted": [3], "all": []}[mode]
        for r in range(XENT_R):
            if r not in keep:
                labels[r] = ignore
    counted = labels != ignore
    x = logits.double()
    cnt = max(int(counted.sum()), 1)
    lse = torch.logsumexp(x, 1)
    safe = labels.clamp(min=0)
    loss = torch.where(counted, lse - x.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse)).sum() / cnt
    onehot = F.one_hot(safe, V).double()
    grad = (torch.softmax(x, 1) - onehot) * counted[:, None] * (XENT_UP / cnt)
    # yardstick: fp32 F.cross_entropy on the fp32 copy (sum over rows / count, NaN-free when all are ignored)
    b = _leaf(logits, dt=F32)
    (F.cross_entropy(b, labels, ignore_index=ignore, reduction="sum") * (XENT_UP / cnt)).backward()
    E = FACTOR * float((b.grad.double() - grad).abs().max())
    return SimpleNamespace(V=V, logits=logits, labels=labels, ignore=ignore, counted=counted, loss=loss, grad=grad,
                           E=E, ninf=ninf, mode=mode)


def xent_run(device, c):
    from gaussiank_sgd_amd.ops import xent
    a = _leaf(c.logits, device)
    labels = c.labels.to(device)
    if is_gpu(device):
        assert xent.fused_available(a)
    loss = xent.cross_entropy(a, labels, c.ignore)
    (loss * XENT_UP).backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    (loss * XENT_UP).backward()
    with torch.no_grad():
        loss_ng = xent.cross_entropy(c.logits.to(device), labels, c.ignore)
    return loss.detach(), g1, a.grad, loss_ng


def xent_check(tally, device, c):
    case = "V=%d ignore=%d %s" % (c.V, c.ignore, c.mode)
    loss, g, g2, loss_ng = xent_run(device, c)
    lerr, lref = abs(float(loss) - float(c.loss)), float(c.loss)
    tally._rec(case, "loss", "2e-5(1+|ref|)", lerr, 2e-5 * (1 + abs(lref)), lerr / (2e-5 * (1 + abs(lref))), 1.0)
    tally.true(case, "loss under no_grad differs", torch.equal(loss_ng, loss) and not loss_ng.requires_grad)
    tally.true(case, "gradient dtype", g.dtype == BF16 and g.shape == c.logits.shape)
    tally.true(case, "second backward differs from the first", torch.equal(g, g2))
    tally.true(case, "NaN in the gradient", not torch.isnan(g).any())
    tally.bf16_out(case, "dlogits", g, c.grad, c.E)
    g = g.float().cpu()
    tally.true(case, "ignored rows must have an exactly zero gradient", not g[~c.counted].any())
    if c.mode == "all":
        tally.true(case, "all rows ignored: loss must be exactly 0.0", float(loss) == 0.0)
        tally.true(case, "all rows ignored: gradient must be all zero", not g.any())
    for r in range(XENT_R):
        if not c.counted[r]:
            continue
        y = int(c.labels[r])
        # the one-hot on the right element: negative at the label (row 5 cancels to -0 or just below),
        # positive at its pair neighbour
        tally.true(case, "row %d: gradient at the label %d is %g" % (r, y, g[r, y]),
                   g[r, y] <= 0 if r == 5 else g[r, y] < 0)
        tally.true(case, "row %d: gradient at the label's pair neighbour %d is %g" % (r, y ^ 1, g[r, y ^ 1]),
                   g[r, y ^ 1] > 0)
        others = torch.ones(c.V, dtype=torch.bool)
        others[y] = False
        tally.true(case, "row %d: a negative gradient off the label" % r, not (g[r][others] < 0).any())
    if c.counted[7]:
        tally.true(case, "-inf logits must get an exactly zero gradient", not g[7, c.ninf].any())


# --------------------------------------------------------------------------- C. embedding

# token counts around the 4-row unroll of emb_sum_rows, kEmbLight = 64 and the 16-token chunks of heavy ids
EMB_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 79, 80, 81, 127, 128, 129)
EMB_V = 301              # 301 = 75 * 4 + 1: the last gather block (4 rows) is ragged
EMB_H = (12, 260, 768, 1024)


@functools.lru_cache(maxsize=None)
def emb_runlength_ids():
    """[4, 256] ids: one id per count of EMB_COUNTS (ids 0 and V - 1 among them), unique filler ids, shuffled."""
    gen = torch.Generator().manual_seed(5)
    pool = torch.randperm(EMB_V - 2, generator=gen) + 1            # 1 .. V-2
    heavy = [0, EMB_V - 1] + pool[:len(EMB_COUNTS) - 2].tolist()   # id 0: 1 token, id V-1: 2 tokens, ...
    heavy[0], heavy[-1] = heavy[-1], heavy[0]                      # ... id 0: 129 tokens
    ids = [i for i, n in zip(heavy, EMB_COUNTS) for _ in range(n)]
    B, T = 4, 256
    fill = B * T - len(ids)
    ids += pool[len(EMB_COUNTS) - 2:len(EMB_COUNTS) - 2 + fill].tolist()
    ids = torch.tensor(ids)[torch.randperm(B * T, generator=gen)].reshape(B, T)
    counts = torch.bincount(ids.reshape(-1), minlength=EMB_V)
    assert sorted(counts[heavy].tolist()) == sorted(EMB_COUNTS) and counts[0] == 129 and counts[EMB_V - 1] == 2
    assert int((counts == 0).sum()) > 50 and int(counts.max()) == 129
    return ids


@functools.lru_cache(maxsize=None)
def emb_case(B, T, V, P, NT, H, tt_kind, ids_kind="random", dy_bf16=False):
    gen = torch.Generator().manual_seed(B * 131 + T * 17 + H + NT)
    ids = emb_runlength_ids() if ids_kind == "runlength" else torch.randint(0, V, (B, T), generator=gen)
    assert ids.shape == (B, T)
    tt = {"none": None, "ones": torch.ones(B, T, dtype=torch.long),
          "random": torch.randint(0, NT, (B, T), generator=gen)}[tt_kind]
    tables = [torch.randn(n, H, generator=gen) for n in (V, P, NT)]
    dy = torch.randn(B, T, H, generator=gen)
    if dy_bf16:
        dy = dy.to(BF16)
    d = dy.double().reshape(-1, H)
    flat, ttf = ids.reshape(-1), (tt.reshape(-1) if tt is not None else torch.zeros(B * T, dtype=torch.long))
    pos = torch.arange(T).repeat(B)
    ref, sumabs, n = [], [], []
    for rows, idx in ((V, flat), (P, pos), (NT, ttf)):
        ref.append(torch.zeros(rows, H, dtype=F64).index_add_(0, idx, d))
        sumabs.append(torch.zeros(rows, H, dtype=F64).index_add_(0, idx, d.abs()))
        n.append(torch.bincount(idx, minlength=rows).double()[:, None])
    return SimpleNamespace(B=B, T=T, V=V, P=P, NT=NT, H=H, ids=ids, tt=tt, tables=tables, dy=dy, ref=ref,
                           sumabs=sumabs, n=n)


def emb_run(device, c, frozen=None, expect_fused=True):
    """bert_embeddings forward + backward on ``device``; ``frozen``: index of the table without a gradient.
    Returns (out, composition of the same tables on the same device, [dWw, dWp, dWt])."""
    from gaussiank_sgd_amd.ops import embedding as emb
    mods = [nn.Embedding(t.shape[0], c.H).to(device) for t in c.tables]
    with torch.no_grad():
        for m, t in zip(mods, c.tables):
            m.weight.copy_(t)
    if frozen is not None:
        mods[frozen].weight.requires_grad_(False)
    ids = c.ids.to(device)
    tt = c.tt.to(device) if c.tt is not None else None
    if is_gpu(device):
        assert emb.fused_available(ids, *mods) == expect_fused
    out = emb.bert_embeddings(ids, tt, *mods)
    dy = c.dy.to(device)
    if dy.dtype == BF16:
        out.to(BF16).backward(dy)     # a bf16 upstream gradient
    else:
        out.backward(dy)
    with torch.no_grad():
        comp = mods[0](ids) + mods[1](torch.arange(c.T, device=device).unsqueeze(0)) + \
            mods[2](tt if tt is not None else torch.zeros_like(ids))
    return out.detach(), comp, [m.weight.grad for m in mods]


def emb_check(tally, case, c, out, comp, grads):
    tally.true(case, "forward is not bit-equal to the composition",
               out.dtype == F32 and out.shape == (c.B, c.T, c.H) and torch.equal(out, comp))
    for name, g, ref, sumabs, n in zip(("dword", "dpos", "dtype"), grads, c.ref, c.sumabs, c.n):
        if g is None:
            continue
        tally.fp32_sum(case, name, g, ref, n, sumabs)
        absent = (n[:, 0] == 0)
        tally.true(case, "%s: rows without a token must be exactly zero" % name, not g.cpu()[absent].any())


# --------------------------------------------------------------------------- D. GELU backward + bias column sum

GELU_M = (1, 7, 9, 65)
GELU_N = (8, 264)
GELU_SPECIAL = (0.0, 1e-3, -1e-3, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0)


@functools.lru_cache(maxsize=None)
def gelu_case(M, N, dt):
    """pre = 4 * randn with whole columns set to the special values: all nine at N = 264; at N = 8 the eight
    columns take eight of them, rotated by the index of M so that the four M cover all nine."""
    gen = torch.Generator().manual_seed(M * 1000 + N)
    pre = 4.0 * torch.randn(M, N, generator=gen)
    rot = GELU_M.index(M)
    for j in range(min(N, len(GELU_SPECIAL))):
        pre[:, j] = GELU_SPECIAL[(j + rot) % len(GELU_SPECIAL)]
    pre = pre.to(dt)
    dy = torch.randn(M, N, generator=gen).to(dt)
    ref = torch.ops.aten.gelu_backward(dy.double(), pre.double())
    y32 = torch.ops.aten.gelu_backward(dy.float(), pre.float())
    return SimpleNamespace(M=M, N=N, dt=dt, pre=pre, dy=dy, ref=ref, y32=y32)


def gelu_check(tally, device, c, with_db):
    from gaussiank_sgd_amd.ops.linear import gelu_backward_
    case = "M=%d N=%d %s%s" % (c.M, c.N, "bf16" if c.dt == BF16 else "fp32", " +db" if with_db else "")
    db = torch.zeros(c.N, dtype=F32, device=device) if with_db else None
    dpre = gelu_backward_(c.dy.to(device), c.pre.to(device), db)
    tally.true(case, "dpre dtype / shape", dpre.dtype == c.dt and dpre.shape == c.pre.shape)
    if c.dt == BF16:
        E = FACTOR * float((c.y32.double() - c.ref).abs().max())
        tally.bf16_out(case, "dpre", dpre, c.ref, E)
    else:
        tally.yard(case, "dpre", dpre, c.ref, c.y32)
    if with_db:
        stored = _cpu64(dpre)
        tally.fp32_sum(case, "db", db, stored.sum(0), c.M, stored.abs().sum(0))


# --------------------------------------------------------------------------- scenarios shared by the CPU and GPU tests

def _cdname(cd):
    return "bf16" if cd == BF16 else "fp32"


def _ln_fused(device, inp):
    """True on a GPU (where the supported sizes must take the HIP path), False for the composition."""
    from gaussiank_sgd_amd.ops import ln as L
    probe = inp.x[:1].to(device)
    if is_gpu(device):
        assert L.fused_available(probe), "H = %d must take the fused path" % inp.H
        return True
    assert not L.fused_available(probe)
    return False


def scenario_ln_edges(device, cd):
    """A1: every (CH, RPW) instance at its lower and upper edge, R in {1, 19}; da bit-equal to dx."""
    t = Tally("A1 ln edges " + _cdname(cd))
    hit = set()
    for nc in A1_NC:
        for R in A1_R:
            inp, r64, r32, rbf = ln_refs(R, 8 * nc, cd)
            fused = _ln_fused(device, inp)
            ours = ln_api(device, inp)
            case = "nc=%d R=%d" % (nc, R)
            ln_check(t, case, ours, inp, r64, r32, rbf, fused=fused)
            t.true(case, "without dropout da must be bit-equal to dx", torch.equal(ours["da"], ours["dx"]))
            t.true(case, "output dtypes", ours["y"].dtype == cd and ours["dx"].dtype == cd and ours["dg"].dtype == F32)
            hit.add(ln_bucket(nc))
    # forward and backward of every case dispatch on the same nc: all seven instances of this storage type ran
    assert hit == {(1, 2), (2, 2), (3, 2), (4, 2), (6, 2), (8, 2), (8, 1)}, hit
    t.finish()


def scenario_ln_finalize(device):
    """A2: 71 partial rows (per = 3: a ragged last split, empty splits after it) and exactly kFinSplits."""
    t = Tally("A2 ln finalize fp32")
    for R in (16 * 70 + 3, 16 * 32):
        P = -(-R // LN_ROWS_PER_BLOCK)
        per = -(-P // LN_FIN_SPLITS)
        assert (P, per) in ((71, 3), (32, 1)) and (P == 32 or (P % per != 0 and per * (LN_FIN_SPLITS - 1) > P))
        inp, r64, r32, rbf = ln_refs(R, 264, F32)
        ln_check(t, "R=%d" % R, ln_api(device, inp), inp, r64, r32, rbf, fused=_ln_fused(device, inp))
    t.finish()


def scenario_ln_offset(device):
    """A3: rows with mean 100 and standard deviation 0.1 (a one-pass variance would lose every digit)."""
    t = Tally("A3 ln offset fp32")
    for H in (264, 4096):
        inp, r64, r32, rbf = ln_refs(19, H, F32, True)
        h = inp.x.double() + inp.a.double()
        assert abs(float(h.mean()) - 100) < 0.1 and abs(float(h.std(1).mean()) - 0.1) < 0.01
        ln_check(t, "H=%d" % H, ln_api(device, inp), inp, r64, r32, rbf, fused=_ln_fused(device, inp))
    t.finish()


def scenario_ln_unsupported(device):
    """A7: H = 4104 (> 4096) and H = 12 (no multiple of 8) take the composition, which must still be right."""
    from gaussiank_sgd_amd.ops import ln as L
    t = Tally("A7 ln unsupported H")
    for H in (4104, 12):
        for cd in (F32, BF16):
            inp, r64, r32, rbf = ln_refs(19, H, cd)
            assert not L.fused_available(inp.x.to(device))
            ln_check(t, "H=%d %s" % (H, _cdname(cd)), ln_api(device, inp), inp, r64, r32, rbf, fused=False)
    t.finish()


def scenario_xent(device, V):
    t = Tally("B xent")
    for ignore, mode in XENT_IGNORE:
        xent_check(t, device, xent_case(V, ignore, mode))
    t.finish()


def scenario_emb_runlength(device, H):
    t = Tally("C emb run lengths")
    c = emb_case(4, 256, EMB_V, 300, 2, H, "random", "runlength")
    emb_check(t, "H=%d" % H, c, *emb_run(device, c))
    t.finish()


def scenario_emb_positions(device, B):
    t = Tally("C emb positions")
    c = emb_case(B, 7, 50, 12, 2, 260, "random")
    out, comp, grads = emb_run(device, c)
    emb_check(t, "B=%d" % B, c, out, comp, grads)
    t.true("B=%d" % B, "position rows T..P-1 must be exactly zero", not grads[1][c.T:].any())
    t.finish()


EMB_TYPE_CASES = {"ones-M257": (1, 257, 2, "ones"), "none-M1100": (4, 275, 2, "none"),
                  "onerow-none-M257": (1, 257, 1, "none"), "random-M1100": (4, 275, 2, "random")}


def scenario_emb_types(device, kind):
    t = Tally("C emb types")
    B, T, NT, tt_kind = EMB_TYPE_CASES[kind]
    c = emb_case(B, T, 50, T, NT, 260, tt_kind)
    out, comp, grads = emb_run(device, c)
    emb_check(t, kind, c, out, comp, grads)
    if tt_kind == "ones":
        t.true(kind, "type row 0 must be exactly zero", not grads[2][0].any() and bool(grads[2][1].any()))
    t.finish()


def scenario_emb_frozen(device):
    """Each table frozen in turn: no gradient for it, the other two bit-equal to the all-trainable run."""
    t = Tally("C emb frozen")
    c = emb_case(4, 256, EMB_V, 300, 2, 260, "random", "runlength")
    out, comp, full = emb_run(device, c)
    emb_check(t, "all trainable", c, out, comp, full)
    for k, name in enumerate(("word", "pos", "type")):
        out_k, _, grads = emb_run(device, c, frozen=k)
        t.true(name, "a frozen table must get no gradient", grads[k] is None)
        t.true(name, "forward changed", torch.equal(out_k, out))
        for j in range(3):
            if j != k:
                t.true(name, "gradient %d differs from the all-trainable run" % j,
                       grads[j] is not None and torch.equal(grads[j], full[j]))
    t.finish()


def scenario_emb_other(device):
    t = Tally("C emb other")
    c = emb_case(2, 40, 50, 64, 2, 768, "random", dy_bf16=True)
    emb_check(t, "bf16 dy", c, *emb_run(device, c))
    c = emb_case(2, 40, 50, 64, 2, 1028, "random")        # H / 4 = 257 > 256: the composition
    emb_check(t, "H=1028", c, *emb_run(device, c, expect_fused=False))
    t.finish()


def scenario_gelu(device, dt):
    from gaussiank_sgd_amd.ops.linear import _colsum_ok
    t = Tally("D gelu bwd " + _cdname(dt))
    for M in GELU_M:
        for N in GELU_N:
            c = gelu_case(M, N, dt)
            assert _colsum_ok(c.pre.to(device)) == is_gpu(device)
            for with_db in (False, True):
                gelu_check(t, device, c, with_db)
    t.finish()


def scenario_empty(device):
    """E: zero rows through all three ops (forward and backward), then an ordinary kernel and a sync."""
    from gaussiank_sgd_amd.ops import embedding as emb
    from gaussiank_sgd_amd.ops import xent
    from gaussiank_sgd_amd.ops.ln import add_layernorm
    logits = torch.zeros(0, 514, dtype=BF16, device=device, requires_grad=True)
    loss = xent.cross_entropy(logits, torch.zeros(0, dtype=torch.long, device=device))
    assert loss.shape == () and float(loss.detach()) == 0.0
    loss.backward()
    assert logits.grad.shape == (0, 514) and logits.grad.dtype == BF16

    mods = [nn.Embedding(n, 64).to(device) for n in (50, 16, 2)]
    ids = torch.zeros(0, 7, dtype=torch.long, device=device)
    for tt in (None, ids.clone()):
        out = emb.bert_embeddings(ids, tt, *mods)
        assert out.shape == (0, 7, 64) and out.dtype == F32
        out.sum().backward()
    for m in mods:
        assert m.weight.grad.shape == m.weight.shape and not m.weight.grad.any()

    for cd in (F32, BF16):
        ln = nn.LayerNorm(264).to(device)
        a = torch.zeros(0, 264, dtype=cd, device=device, requires_grad=True)
        x = torch.zeros(0, 264, dtype=cd, device=device, requires_grad=True)
        y = add_layernorm(a, x, ln, 0.1, True)
        assert y.shape == (0, 264) and y.dtype == cd
        y.sum().backward()
        assert x.grad.shape == (0, 264) and a.grad.shape == (0, 264)
        assert ln.weight.grad.shape == (264,) and not ln.weight.grad.any() and not ln.bias.grad.any()

    z = torch.ones(1000, device=device) * 2      # an ordinary kernel after them: no launch error left behind
    if is_gpu(device):
        torch.cuda.synchronize()
    assert float(z.sum()) == 2000.0
