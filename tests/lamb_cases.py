"""Shared cases of the fused LAMB tests (tests/test_lamb_cpu.py runs them on the
pure-torch fallback of ``ops.fused_lamb_``, tests/test_lamb_gpu.py on the HIP
kernels).  Shapes, arena layout, gradients and the tolerance rule come from
tests/adam_cases.py unchanged.

Yardstick.  ``lamb_plain`` below is a plain per-tensor implementation of the
LAMB formula in torch ops, parametrised by dtype; it shares no code with
``optim.LAMB.step`` or the op's fallback.  It runs at fp64 and at fp32 on the
same inputs; after every step the max-abs error of ours against the fp64 run,
for each of ``w``, ``m``, ``v``, must be <= ``adam_cases.FACTOR`` (2) times the
fp32-vs-fp64 difference (room for FMA contraction and operation order).

Trust ratios.  ``ws.trust`` against the fp64 run within a relative
``TRUST_RTOL = 2e-5``, derived for the kernel's block of 256 threads over a
chunk of at most 16384 elements: each lane adds at most 16384 / 256 = 64 fp32
squares (gamma_64 ~ 64 * 2^-24 ~ 4e-6 on a sum of squares, half that on the
norm), everything across lanes, waves and chunks is added in double; on top
come the fp32 rounding of every ``u`` (a few 2^-24 per element, a few 1e-7 on
the norm at worst), the two fp32 square roots and the fp32 divide (2e-7
together): about 3e-6 for each norm in the worst case, 6e-6 for the ratio,
times a safety factor of 3.  Re-derive it if the block size or the chunk size
changes.
"""
import functools
import math

import torch

import adam_cases as ac
from gaussiank_sgd_amd import ops

GROUP_OF = ac.GROUP_OF                # tensor -> param group: (1000, 64), the 4-chunk tensor, alone in group 2
STEPS_MAX = ac.STEPS_MAX
TRUST_RTOL = 2e-5
CLIP = 0.25
# "mixed": group 0 adapts, group 1 does not, group 2 adapts under a clip that binds (the test asserts it does);
# "adaptall": every tensor adapts, no clip; "noadapt": adam_cases.HYPER with adapt off = AdamW
VARIANTS = {
    "mixed": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True, trust_clip=None),
              dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, adapt=False, trust_clip=None),
              dict(lr=5e-4, betas=(0.95, 0.995), eps=1e-8, weight_decay=0.1, adapt=True, trust_clip=CLIP)],
    "adaptall": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True, trust_clip=None),
                 dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, adapt=True, trust_clip=None),
                 dict(lr=5e-4, betas=(0.95, 0.995), eps=1e-8, weight_decay=0.1, adapt=True, trust_clip=None)],
    "noadapt": [dict(h, adapt=False, trust_clip=None) for h in ac.HYPER],
}
CASES = [(v, s) for v in ("mixed", "adaptall") for s in (False, True)]
CASE_IDS = ["%s-%s" % (v, "sparse1pct" if s else "dense") for v, s in CASES]
PADDED_LENS = [ac._pad(n) for n in ac.NUMELS]


def chunk_table(device, lens=None, group_of=None):
    """adam_cases.chunk_table with a choice of the tensor -> group map."""
    lens = PADDED_LENS if lens is None else lens
    group_of = GROUP_OF if group_of is None else group_of
    return ops.make_chunk_table([(o, ln, g, i) for i, (o, ln, g) in enumerate(zip(ac.OFFSETS, lens, group_of))],
                                device)


def lamb_plain(w0, grads, lens, hyper, dtype, gs=1.0, lm=1.0, group_of=None):
    """The yardstick: LAMB per tensor on the slots [offset, offset + len) of flat arenas, in ``dtype``.
    Returns per step {"w", "m", "v"} (fp64 arenas) and "trust" (one float per tensor)."""
    group_of = GROUP_OF if group_of is None else group_of
    w = w0.to(dtype).clone()
    m = torch.zeros_like(w)
    v = torch.zeros_like(w)
    out = []
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        trusts = []
        for i, (o, ln) in enumerate(zip(ac.OFFSETS, lens)):
            h = hyper[group_of[i]]
            b1, b2 = h["betas"]
            wi, mi, vi = w[o:o + ln], m[o:o + ln], v[o:o + ln]
            d = g[o:o + ln] * gs
            mi += (1.0 - b1) * (d - mi)
            vi *= b2
            vi += (1.0 - b2) * d * d
            u = (mi / (1.0 - b1 ** t)) / (vi.sqrt() / math.sqrt(1.0 - b2 ** t) + h["eps"]) + h["weight_decay"] * wi
            wn, un = torch.sqrt((wi * wi).sum()), torch.sqrt((u * u).sum())
            trust = float(wn / un) if h["adapt"] and wn > 0 and un > 0 else 1.0
            if h["trust_clip"]:
                trust = min(trust, h["trust_clip"])
            wi -= (h["lr"] * lm * trust) * u
            trusts.append(trust)
        out.append({"w": w.double().clone(), "m": m.double().clone(), "v": v.double().clone(), "trust": trusts})
    return out


@functools.lru_cache(maxsize=None)
def inputs(sparse):
    w0, grads = ac.make_inputs(sparse)
    return ac.to_arena(w0), [ac.to_arena(g) for g in grads]


@functools.lru_cache(maxsize=None)
def reference(variant, sparse, ragged=False, gs=1.0, lm=1.0):
    """(w0 arena, gradient arenas as fed to the op, fp64 run, fp32 run); the gradients are divided by
    ``gs`` (in fp32) so that the op's grad_scale restores them."""
    w0, grads = inputs(sparse)
    if gs != 1.0:
        grads = [g / gs for g in grads]
    lens = ac.RAGGED_LENS if ragged else PADDED_LENS
    r64 = lamb_plain(w0, grads, lens, VARIANTS[variant], torch.float64, gs, lm)
    r32 = lamb_plain(w0, grads, lens, VARIANTS[variant], torch.float32, gs, lm)
    return w0, grads, r64, r32


def check_trust(label, trust, ref64):
    worst = 0.0
    got = trust.detach().cpu().double().tolist()
    for i, (a, b) in enumerate(zip(got, ref64["trust"])):
        rel = abs(a - b) / abs(b)
        worst = max(worst, rel)
        assert rel <= TRUST_RTOL, "%s tensor %d: trust %.9g against %.9g (fp64), relative %.3e > %.1e" % (
            label, i, a, b, rel, TRUST_RTOL)
    print("%s trust %s largest relative error %.3e" % (label, ["%.4g" % x for x in got], worst))
    return worst


class State:
    def __init__(self, w0, device, with_shadow=False, lens=None, group_of=None):
        dev = torch.device(device)
        self.w = w0.clone().to(dev)
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self.step = torch.zeros((), dtype=torch.float32, device=dev)
        self.shadow = torch.zeros(ac.TOTAL, dtype=torch.bfloat16, device=dev) if with_shadow else None
        self.chunks = chunk_table(dev, lens, group_of)
        self.ws = ops.make_lamb_workspace(self.chunks, dev)

    def run(self, g, groups, **kw):
        ops.fused_lamb_(self.w, self.m, self.v, g, self.chunks, groups, self.step, self.ws, w_bf16=self.shadow, **kw)

    def tensors(self):
        return {"w": self.w, "m": self.m, "v": self.v, "trust": self.ws.trust, "step": self.step}


def run_case(variant, sparse, steps, device, with_shadow=False, on_step=None, ragged=False, gs=1.0, lm=1.0):
    """``steps`` calls of ops.fused_lamb_ on ``device``; the 2x rule and the trust ratios after every step."""
    w0, grads, r64, r32 = reference(variant, sparse, ragged, gs, lm)
    lens = ac.RAGGED_LENS if ragged else None
    mask = ac.covered_mask(lens) if ragged else None
    st = State(w0, device, with_shadow, lens)
    dev = st.w.device
    g = torch.zeros_like(st.w)
    kw = {}
    if gs != 1.0:
        kw["grad_scale"] = torch.full((1,), gs, device=dev)
    if lm != 1.0:
        kw["lr_mult"] = torch.full((1,), lm, device=dev)
    worst = worst_trust = 0.0
    for t in range(steps):
        g.copy_(grads[t])
        st.run(g, VARIANTS[variant], zero_grad=True, **kw)
        label = "lamb %s/%s%s step %d" % (variant, "sparse" if sparse else "dense", "/ragged" if ragged else "", t + 1)
        worst = max(worst, ac.check_step(label, {"w": st.w, "m": st.m, "v": st.v}, r64[t], r32[t], mask))
        worst_trust = max(worst_trust, check_trust(label, st.ws.trust, r64[t]))
        assert torch.isfinite(st.w).all() and torch.isfinite(st.m).all() and torch.isfinite(st.v).all()
        if on_step is not None:
            on_step(t, st, g)
    assert float(st.step) == steps
    print("lamb %s/%s%s: largest w/m/v ratio %.3f, largest trust error %.3e" % (
        variant, "sparse" if sparse else "dense", "/ragged" if ragged else "", worst, worst_trust))
    return worst, r64


# ---------------------------------------------------------------------------
# the cases, each taking the device
# ---------------------------------------------------------------------------
def case_yardstick(variant, sparse, device):
    """8 steps on the arena's padded layout: the rule, the ratios, zeroed gradients, the shadow, padding."""
    pad = ac.padding_mask().to(device)

    def on_step(t, st, g):
        assert not g.any(), "the gradient arena is zeroed in the apply pass"
        assert torch.equal(st.shadow, st.w.to(torch.bfloat16))
        assert not st.w[pad].any() and not st.m[pad].any() and not st.v[pad].any(), "padding must stay exactly 0"

    worst, r64 = run_case(variant, sparse, STEPS_MAX, device, with_shadow=True, on_step=on_step)
    if variant == "mixed":
        # the yardstick itself: the clip binds on the 4-chunk tensor, group 1 does not adapt, group 0 does
        assert all(r["trust"][2] == CLIP for r in r64)
        assert all(r["trust"][1] == 1.0 and r["trust"][3] == 1.0 for r in r64)
        assert all(r["trust"][0] != 1.0 and r["trust"][4] != 1.0 for r in r64)
    elif not sparse:       # (a sparse gradient may leave a wd = 0 tensor with u = 0: ratio 1)
        assert all(x != 1.0 for r in r64 for x in r["trust"])
    return worst


def case_noadapt_is_adamw(sparse, device):
    """adapt off in every group: torch.optim.AdamW(foreach=False) at fp64 / fp32 is the yardstick."""
    w0, grads, r64, r32 = ac.reference("adamw", sparse)
    st = State(w0, device)
    g = torch.zeros_like(st.w)
    worst = 0.0
    for t in range(STEPS_MAX):
        g.copy_(grads[t])
        st.run(g, VARIANTS["noadapt"])
        worst = max(worst, ac.check_step("lamb noadapt vs AdamW/%s step %d" % ("sparse" if sparse else "dense", t + 1),
                                         {"w": st.w, "m": st.m, "v": st.v}, r64[t], r32[t]))
        assert torch.equal(st.ws.trust, torch.ones_like(st.ws.trust))
    print("lamb noadapt vs AdamW/%s largest ratio %.3f" % ("sparse" if sparse else "dense", worst))
    return worst


def case_degenerate(device):
    """Tensor 0: all-zero weights; 1: all-zero gradients at step 1 with wd = 0; 2: both; 3: an ordinary one.
    Every one adapts.  Lengths 100 / 64 / 7 / 300: 7 leaves 57 slots the table does not cover."""
    dev = torch.device(device)
    lens, offs = [100, 64, 7, 300], [0, 128, 192, 256]
    total = 576
    chunks = ops.make_chunk_table([(o, ln, 0, i) for i, (o, ln) in enumerate(zip(offs, lens))], dev)
    ws = ops.make_lamb_workspace(chunks, dev)
    gen = torch.Generator().manual_seed(5)
    w = torch.zeros(total)
    g = torch.zeros(total)
    g[0:100] = torch.randn(100, generator=gen)
    w[128:192] = torch.randn(64, generator=gen)
    w[256:556] = torch.randn(300, generator=gen)
    g[256:556] = torch.randn(300, generator=gen)
    w, g = w.to(dev), g.to(dev)
    w0 = w.clone()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    step = torch.zeros((), dtype=torch.float32, device=dev)
    groups = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, adapt=True, trust_clip=None)]
    ops.fused_lamb_(w, m, v, g, chunks, groups, step, ws)
    trust = ws.trust.cpu().tolist()
    print("degenerate trust", trust)
    assert trust[0] == 1.0 and trust[1] == 1.0 and trust[2] == 1.0
    assert trust[3] != 1.0 and math.isfinite(trust[3])
    for x in (w, m, v, ws.trust):
        assert torch.isfinite(x).all()
    assert w[0:100].any(), "zero weights with gradients still move (trust 1)"
    assert torch.equal(w[128:192], w0[128:192]) and torch.equal(w[192:256], w0[192:256]), "u = 0: w bit-unchanged"
    assert not torch.equal(w[256:556], w0[256:556])
    assert float(step) == 1.0


def case_ragged(variant, sparse, device):
    """adam_cases.run_ragged for LAMB: norms over the covered slots, everything beyond a length untouched."""
    inside = ac.covered_mask(ac.RAGGED_LENS).to(device)
    w0, grads, _, _ = reference(variant, sparse, True)
    w0d = w0.to(device)

    def on_step(t, st, g):
        assert not g[inside].any(), "covered gradients are zeroed"
        assert torch.equal(g[~inside], grads[t].to(device)[~inside]), "gradients beyond a chunk's length were touched"
        assert torch.equal(st.shadow[inside], st.w[inside].to(torch.bfloat16))
        assert not st.shadow[~inside].any(), "shadow beyond a chunk's length was written"
        assert torch.equal(st.w[~inside], w0d[~inside]), "w beyond a chunk's length was touched"
        assert not st.m[~inside].any() and not st.v[~inside].any(), "moments beyond a chunk's length were touched"
        assert st.m[inside].any() and st.v[inside].any()

    return run_case(variant, sparse, 4, device, with_shadow=True, on_step=on_step, ragged=True)[0]


def _advance(st, grads, groups, lo, hi, **kw):
    for t in range(lo, hi):
        st.run(grads[t].clone().to(st.w.device), groups, **kw)


def case_zero_grad_false(device):
    w0, grads = inputs(False)
    a, b = State(w0, device), State(w0, device)
    groups = VARIANTS["mixed"]
    for t in range(3):
        ga, gb = grads[t].clone().to(device), grads[t].clone().to(device)
        a.run(ga, groups, zero_grad=True)
        b.run(gb, groups, zero_grad=False)
        assert not ga.any()
        assert torch.equal(gb, grads[t].to(device)), "zero_grad=False must leave g bit-unchanged"
        for k, x in a.tensors().items():
            assert torch.equal(x, b.tensors()[k]), k


def case_device_scalars(device, bitwise_lr_mult=True):
    w0, grads = inputs(False)
    groups = VARIANTS["mixed"]
    half = [dict(h, lr=h["lr"] * 0.5) for h in groups]
    a, b = State(w0, device), State(w0, device)
    _advance(a, grads, groups, 0, 3, lr_mult=torch.full((1,), 0.5, device=device))
    _advance(b, grads, half, 0, 3)
    assert float(a.step) == 3.0 and float(b.step) == 3.0
    for k, x in a.tensors().items():
        assert torch.equal(x, b.tensors()[k]), "lr_mult = 0.5 against halved lr: %s differs" % k
    # lr_mult = 0: the moments and the ratios move, the weights do not
    c = State(w0, device)
    _advance(c, grads, groups, 0, 1, lr_mult=torch.zeros(1, device=device))
    assert torch.equal(c.w, w0.to(device)) and c.m.any() and c.v.any()
    # grad_scale: gradients divided by 0.37 and restored by the op, under the rule (the yardstick scales too)
    return run_case("mixed", False, 4, device, gs=0.37)[0]


def case_determinism(device):
    """Two runs from the same state, and a run with the group ids permuted (same hyper-parameters per tensor)."""
    w0, grads = inputs(True)
    groups = VARIANTS["mixed"]
    perm = [2, 0, 1]                                   # old group id -> new group id
    pgroups = [groups[perm.index(i)] for i in range(3)]
    runs = [State(w0, device), State(w0, device), State(w0, device, group_of=[perm[g] for g in GROUP_OF])]
    for t in range(STEPS_MAX):
        for st, gr in zip(runs, (groups, groups, pgroups)):
            st.run(grads[t].clone().to(device), gr)
        for other, what in ((runs[1], "second run"), (runs[2], "permuted group ids")):
            for k, x in runs[0].tensors().items():
                assert torch.equal(x, other.tensors()[k]), "step %d, %s: %s differs" % (t + 1, what, k)
