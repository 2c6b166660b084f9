"""Shared cases of the fused Adam / AdamW tests (tests/test_adam_cpu.py runs
them on the pure-torch fallback of ``ops.fused_adam_``, tests/test_adam_gpu.py
on the HIP kernel).

Tolerance rule.  The yardstick is torch's own rounding, not the code under
test: ``torch.optim.Adam(W)`` in fp32 against the same optimizer in fp64 on
the same inputs, max abs difference over the whole arena, for each of ``w``,
``exp_avg`` and ``exp_avg_sq`` after every step (over the slots the chunk
table covers, when a case passes lengths of its own).  Ours against the same
fp64 run must stay within 2x that (room for FMA contraction and operation
order; a plain fp32 implementation of the formula lands at about 1x).  The
torch runs are computed once per (variant, gradient kind) and shared.
"""
import functools

import torch

from gaussiank_sgd_amd import ops

SHAPES = [(64, 3, 3, 3), (64,), (1000, 64), (1000,), (7,)]
GROUP_OF = [0, 1, 2, 1, 0]            # tensor -> param group
STEPS_MAX = 8
FACTOR = 2.0
# three groups with different lr / betas / eps / wd
HYPER = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
         dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
         dict(lr=5e-4, betas=(0.95, 0.995), eps=1e-8, weight_decay=0.1)]
# variant -> (torch class, decoupled flag per group)
VARIANTS = {"adamw": (torch.optim.AdamW, [True, True, True]),
            "adam": (torch.optim.Adam, [False, False, False])}
if "decoupled_weight_decay" in torch.optim.Adam([torch.zeros(1)]).defaults:
    # torch's Adam takes the flag per param group: decoupled and coupled groups in one launch
    # (group 2, wd 0.1, is the coupled one that decays; group 0, wd 0.01, the decoupled one)
    VARIANTS["mixed"] = (torch.optim.Adam, [True, False, False])
CASES = [(v, s) for v in VARIANTS for s in (False, True)]
CASE_IDS = ["%s-%s" % (v, "sparse1pct" if s else "dense") for v, s in CASES]


def _pad(n):
    return (n + 63) // 64 * 64


NUMELS = [int(torch.Size(s).numel()) for s in SHAPES]
OFFSETS = [sum(_pad(n) for n in NUMELS[:i]) for i in range(len(NUMELS))]
TOTAL = sum(_pad(n) for n in NUMELS)


def groups_for(variant):
    return [dict(h, decoupled=d) for h, d in zip(HYPER, VARIANTS[variant][1])]


# Lengths that are no multiple of 4, at the same 64-aligned starts: what the public op accepts beyond the
# arena's padded layout.  Every chunk ends in the kernel's scalar tail: 1727 = 431 float4 + 3, 63 = 15 + 3,
# 63999 = three full chunks and one of 14847 = 3711 float4 + 3, 1001 = 250 + 1 (one padding slot), 7 = 1 + 3.
RAGGED_LENS = [1727, 63, 63999, 1001, 7]


def chunk_table(device, lens=None):
    """Default: every tensor padded to 64 elements, as the arena lays them out ((1000, 64) spans 4
    chunks, every length a multiple of 64: float4 path only).  ``lens``: explicit segment lengths."""
    lens = [_pad(n) for n in NUMELS] if lens is None else lens
    return ops.make_chunk_table([(o, ln, g, i) for i, (o, ln, g) in enumerate(zip(OFFSETS, lens, GROUP_OF))],
                                device)


def covered_mask(lens):
    m = torch.zeros(TOTAL, dtype=torch.bool)
    for o, ln in zip(OFFSETS, lens):
        m[o:o + ln] = True
    return m


def to_arena(tensors, dtype=torch.float32):
    a = torch.zeros(TOTAL, dtype=dtype)
    for t, o, n in zip(tensors, OFFSETS, NUMELS):
        a[o:o + n] = t.reshape(-1).to(dtype)
    return a


def padding_mask():
    m = torch.ones(TOTAL, dtype=torch.bool)
    for o, n in zip(OFFSETS, NUMELS):
        m[o:o + n] = False
    return m


def make_inputs(sparse, seed=1234):
    """Initial weights and STEPS_MAX gradients spanning 1e-6 .. 10; ``sparse``: a fresh 1 % mask every
    step (the sparsified aggregate: entries that are non-zero once and zero afterwards)."""
    gen = torch.Generator().manual_seed(seed + int(sparse))
    w0 = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = []
    for _ in range(STEPS_MAX):
        step = []
        for s in SHAPES:
            g = torch.randn(s, generator=gen) * 10.0 ** (torch.rand(s, generator=gen) * 7.0 - 6.0)
            if sparse:
                g = g * (torch.rand(s, generator=gen) < 0.01)
            step.append(g)
        grads.append(step)
    return w0, grads


def _torch_run(variant, w0, grads, dtype):
    cls, dec = VARIANTS[variant]
    params = [w.to(dtype).clone().requires_grad_(True) for w in w0]
    pgs = []
    for gi, h in enumerate(HYPER):
        pg = dict(h, params=[p for p, g in zip(params, GROUP_OF) if g == gi])
        if variant == "mixed":
            pg["decoupled_weight_decay"] = dec[gi]
        pgs.append(pg)
    opt = cls(pgs, foreach=False)
    out = []
    for step in grads:
        for p, g in zip(params, step):
            p.grad = g.to(dtype).clone()
        opt.step()
        out.append({"w": to_arena([p.detach() for p in params], torch.float64),
                    "m": to_arena([opt.state[p]["exp_avg"] for p in params], torch.float64),
                    "v": to_arena([opt.state[p]["exp_avg_sq"] for p in params], torch.float64)})
    return out


@functools.lru_cache(maxsize=None)
def reference(variant, sparse):
    """(w0 arena, gradient arenas, per step {"w","m","v"} of torch fp64, the same of torch fp32)."""
    w0, grads = make_inputs(sparse)
    r64 = _torch_run(variant, w0, grads, torch.float64)
    r32 = _torch_run(variant, w0, grads, torch.float32)
    return to_arena(w0), [to_arena(g) for g in grads], r64, r32


def check_step(label, ours, ref64, ref32, mask=None):
    """ours: {"w","m","v"} fp32 arenas (any device); ref64 / ref32: torch's fp64 and fp32 runs (the
    yardstick is their difference); ``mask``: compare these slots only.  Returns the largest ratio."""
    worst = 0.0
    sel = (lambda t: t[mask]) if mask is not None else (lambda t: t)
    yard = {k: float(sel(ref32[k].double() - ref64[k]).abs().max()) for k in ("w", "m", "v")}
    for k in ("w", "m", "v"):
        err = float(sel(ours[k].detach().cpu().double() - ref64[k]).abs().max())
        ratio = err / yard[k] if yard[k] > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3e yardstick %.3e ratio %.3f" % (label, k, err, yard[k], ratio))
        assert err <= FACTOR * yard[k], "%s %s: err %.3e is %.3f x the torch fp32-vs-fp64 yardstick %.3e (limit %gx)" % (
            label, k, err, ratio, yard[k], FACTOR)
        worst = max(worst, ratio)
    return worst


def run_case(variant, sparse, steps, device, with_shadow=False, on_step=None, lens=None):
    """``steps`` calls of ops.fused_adam_ on ``device`` checked against the rule after every step.
    ``lens``: explicit chunk-table lengths (the rule then covers the slots inside them)."""
    w0, grads, r64, r32 = reference(variant, sparse)
    mask = covered_mask(lens) if lens is not None else None
    dev = torch.device(device)
    w = w0.clone().to(dev)
    m = torch.zeros_like(w)
    v = torch.zeros_like(w)
    g = torch.zeros_like(w)
    step = torch.zeros((), dtype=torch.float32, device=dev)
    shadow = torch.zeros(TOTAL, dtype=torch.bfloat16, device=dev) if with_shadow else None
    chunks = chunk_table(dev, lens)
    groups = groups_for(variant)
    worst = 0.0
    for t in range(steps):
        g.copy_(grads[t])
        ops.fused_adam_(w, m, v, g, chunks, groups, step, zero_grad=True, w_bf16=shadow)
        label = "%s/%s step %d" % (variant, "sparse" if sparse else "dense", t + 1)
        worst = max(worst, check_step(label, {"w": w, "m": m, "v": v}, r64[t], r32[t], mask))
        if on_step is not None:
            on_step(t, w, m, v, g, step, shadow)
    assert float(step) == steps
    return worst


def run_ragged(variant, sparse, steps, device):
    """RAGGED_LENS through ops.fused_adam_: the rule on the covered slots, their gradients zeroed and
    their shadow equal to bf16(w); every slot beyond a chunk's length untouched in w, m, v, g and the shadow."""
    w0, grads, _, _ = reference(variant, sparse)
    dev = torch.device(device)
    inside = covered_mask(RAGGED_LENS).to(dev)
    w0 = w0.to(dev)

    def on_step(t, w, m, v, g, step, shadow):
        assert not g[inside].any(), "covered gradients are zeroed"
        assert torch.equal(g[~inside], grads[t].to(dev)[~inside]), "gradients beyond a chunk's length were touched"
        assert torch.equal(shadow[inside], w[inside].to(torch.bfloat16))
        assert not shadow[~inside].any(), "shadow beyond a chunk's length was written"
        assert torch.equal(w[~inside], w0[~inside]), "w beyond a chunk's length was touched"
        assert not m[~inside].any() and not v[~inside].any(), "moments beyond a chunk's length were touched"
        assert m[inside].any() and v[inside].any()

    return run_case(variant, sparse, steps, device, with_shadow=True, on_step=on_step, lens=RAGGED_LENS)
