"""Shared cases of the arena kernels that stream a chunk table (fused SGD, DGC
momentum correction, the LARS norms and update): tests/test_arena_cpu.py runs
them on the pure-torch fallbacks, tests/test_arena_kernels_gpu.py on the HIP
kernels.  Fused Adam and LAMB have cases of their own (adam_cases.py,
lamb_cases.py).

Every case uses LENS at the 64-aligned starts of ``adam_cases.OFFSETS``: 1727 =
431 float4 + 3, 63 = 15 + 3, 16387 = one full 16384-element chunk and a chunk of
3 (no float4 iteration at all), 1001 = 250 + 1, 7 = 1 + 3, so every chunk ends
in the kernels' scalar tail.  The rule of every case: on the covered slots the
result on ``device`` equals the op's own CPU fallback within the tolerance the
op's older test uses, and every slot beyond a chunk's length is bit-unchanged in
every arena the op writes.
"""
import torch

import adam_cases as ac
from gaussiank_sgd_amd import ops

LENS = [1727, 63, 16387, 1001, 7]
INSIDE = ac.covered_mask(LENS)
# the three groups of test_fused_sgd_vs_torch and one without momentum (it never reads or writes m)
SGD_GROUPS = [dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False),
              dict(lr=0.05, momentum=0.875, dampening=0.1, weight_decay=0.0, nesterov=False),
              dict(lr=0.02, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True),
              dict(lr=0.03, momentum=0.0, dampening=0.0, weight_decay=1e-3, nesterov=False)]
SGD_GROUP_OF = [0, 1, 2, 3, 1]
MC_GROUPS = [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.5, weight_decay=0.0)]
MC_GROUP_OF = [0, 1, 0, 1, 0]
LARS_GROUPS = [dict(lr=0.1, momentum=0.9, weight_decay=5e-4, eeta=1e-3, epsilon=1e-5),
               dict(lr=0.05, momentum=0.8, weight_decay=0.0, eeta=2e-3, epsilon=1e-6),
               dict(lr=0.2, momentum=0.95, weight_decay=1e-3, eeta=1e-3, epsilon=1e-5)]
# Each lane of segmented_sumsq adds at most 64 squares in fp32 before anything is double: 16 float4 iterations, each
# (x^2 + y^2) + (z^2 + w^2) added to the lane's partial, and at most one tail square.  A term goes through one
# rounding of its square, two of the pair sums and at most 17 of the partial; all terms are >= 0, so the partial is
# within 20 * 2^-24 of its exact value, relative, and so is their sum (the double part adds about 1e-14).
SUMSQ_RTOL = 20 * 2.0 ** -24


def table(device, group_of):
    return ops.make_chunk_table([(o, ln, g, i) for i, (o, ln, g) in enumerate(zip(ac.OFFSETS, LENS, group_of))],
                                device)


def _randn(gen, n=1):
    return [torch.randn(ac.TOTAL, generator=gen) for _ in range(n)]


def _check(label, got, want, before, atol, rtol):
    """got (any device) against the fallback's ``want`` inside the chunks, bit-equal to ``before`` beyond them."""
    got = got.cpu()
    assert torch.equal(got[~INSIDE], before[~INSIDE]), "%s: a slot beyond a chunk's length was touched" % label
    assert torch.allclose(got[INSIDE], want[INSIDE], atol=atol, rtol=rtol), "%s: max abs diff %.3e" % (
        label, float((got[INSIDE] - want[INSIDE]).abs().max()))


def run_sgd(device, atol=1e-6, rtol=1e-5):
    """Three steps (first_step on step 0) with shadow and zeroed gradients, a fourth with grad_scale = 0.5 and
    lr_mult = 0.25 as device scalars; then one step of a table without momentum and m=None."""
    dev = torch.device(device)
    gen = torch.Generator().manual_seed(7)
    w0, m0, s0 = _randn(gen, 3)
    s0 = s0.to(torch.bfloat16)
    grads = _randn(gen, 5)

    def step(st, d, t, group_of, groups, m_key="m", **scalars):
        g = grads[t].clone().to(d)
        kw = {k: torch.full((1,), x, device=d) for k, x in scalars.items()}
        ops.fused_sgd_(st["w"], st.get(m_key), g, table(d, group_of), groups, zero_grad=True, w_bf16=st["shadow"],
                       **kw)
        return g

    def check(t, got, want, g):
        for k, before in (("w", w0), ("m", m0)):
            _check("sgd step %d %s" % (t, k), got[k], want[k], before, atol, rtol)
        assert not g[INSIDE].any(), "covered gradients are zeroed"
        assert torch.equal(g[~INSIDE], grads[t][~INSIDE]), "gradients beyond a chunk's length were touched"
        sh = got["shadow"].cpu()
        assert torch.equal(sh[INSIDE], got["w"].cpu()[INSIDE].to(torch.bfloat16))
        assert torch.equal(sh[~INSIDE], s0[~INSIDE]), "shadow beyond a chunk's length was written"

    got = {"w": w0.clone().to(dev), "m": m0.clone().to(dev), "shadow": s0.clone().to(dev)}
    want = {"w": w0.clone(), "m": m0.clone(), "shadow": s0.clone()}
    for t in range(4):
        groups = [dict(p, first_step=(t == 0)) for p in SGD_GROUPS]
        scalars = dict(grad_scale=0.5, lr_mult=0.25) if t == 3 else {}
        g = step(got, dev, t, SGD_GROUP_OF, groups, **scalars)
        step(want, "cpu", t, SGD_GROUP_OF, groups, **scalars)
        check(t, got, want, g.cpu())
    no_m = SGD_GROUP_OF.index(3)
    assert torch.equal(got["m"].cpu()[ac.OFFSETS[no_m]:ac.OFFSETS[no_m] + LENS[no_m]],
                       m0[ac.OFFSETS[no_m]:ac.OFFSETS[no_m] + LENS[no_m]]), "a group without momentum wrote m"
    g = step(got, dev, 4, [0] * 5, SGD_GROUPS[3:], m_key=None)
    step(want, "cpu", 4, [0] * 5, SGD_GROUPS[3:], m_key=None)
    check(4, got, want, g.cpu())


def run_momentum_correct(device, atol=1e-6, rtol=1e-6):
    """Chunks [1, nchunks): the first chunk stays untouched, like every slot beyond a chunk's length."""
    dev = torch.device(device)
    gen = torch.Generator().manual_seed(8)
    u0, g0, w0 = _randn(gen, 3)
    chunks = table(dev, MC_GROUP_OF)
    n = chunks.numel() // 2
    u, g = u0.clone().to(dev), g0.clone().to(dev)
    uc, gc = u0.clone(), g0.clone()
    ops.momentum_correct_(u, g, w0.to(dev), chunks, 1, n - 1, MC_GROUPS)
    ops.momentum_correct_(uc, gc, w0.clone(), table("cpu", MC_GROUP_OF), 1, n - 1, MC_GROUPS)
    _check("momentum_correct u", u, uc, u0, atol, rtol)
    _check("momentum_correct g", g, gc, g0, atol, rtol)
    first = slice(ac.OFFSETS[0], ac.OFFSETS[0] + LENS[0])
    assert torch.equal(u.cpu()[first], u0[first]) and torch.equal(g.cpu()[first], g0[first]), "chunk 0 was touched"
    assert not torch.equal(uc[INSIDE], u0[INSIDE])


def run_lars(device, atol=1e-5, rtol=1e-5):
    """segmented_sumsq_ (its float64 sums within SUMSQ_RTOL of the fallback's), then fused_lars_ from them; two steps."""
    dev = torch.device(device)
    gen = torch.Generator().manual_seed(9)
    w0, m0 = _randn(gen, 2)
    grads = _randn(gen, 2)
    got = {"w": w0.clone().to(dev), "m": m0.clone().to(dev)}
    want = {"w": w0.clone(), "m": m0.clone()}
    worst = 0.0
    cpu = torch.device("cpu")
    for t, g in enumerate(grads):
        # the sums are checked against the fallback's sums of the SAME weights (a host copy of the device's)
        ss = torch.zeros(2 * len(LENS), dtype=torch.float64, device=dev)
        ref = torch.zeros(2 * len(LENS), dtype=torch.float64)
        ops.segmented_sumsq_(got["w"], g.to(dev), table(dev, ac.GROUP_OF), ss)
        ops.segmented_sumsq_(got["w"].cpu(), g, table(cpu, ac.GROUP_OF), ref)
        rel = float(((ss.cpu() - ref).abs() / ref).max())
        worst = max(worst, rel)
        print("segmented_sumsq step %d: largest relative error %.3e (bound %.3e)" % (t, rel, SUMSQ_RTOL))
        assert rel <= SUMSQ_RTOL
        ops.fused_lars_(got["w"], got["m"], g.to(dev), table(dev, ac.GROUP_OF), ss, LARS_GROUPS)
        ss = torch.zeros(2 * len(LENS), dtype=torch.float64)
        ops.segmented_sumsq_(want["w"], g, table(cpu, ac.GROUP_OF), ss)
        ops.fused_lars_(want["w"], want["m"], g, table(cpu, ac.GROUP_OF), ss, LARS_GROUPS)
        for k, before in (("w", w0), ("m", m0)):
            _check("lars step %d %s" % (t, k), got[k], want[k], before, atol, rtol)
    return worst
