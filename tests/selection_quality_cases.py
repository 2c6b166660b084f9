"""Shared cases of the selection-quality tests (tests/test_selection_quality_cpu.py
runs them on the pure-torch mirror, tests/test_selection_quality_gpu.py on the
HIP kernels).

Every case runs ``ops.compress_`` first and ``ops.selection_quality_`` on its
outputs, then compares with an independent fp64 reference written here:
materialise ``acc`` from the residual and the record, ``torch.sort`` it.  The
integer fields (K, c_gt, overlap, sent, k_eff) must match exactly, the energy
fields to relative 1e-5 (the tolerance of the statistics pass,
tests/test_kernels_gpu.py::test_gaussian_pipeline).
"""
import math

import torch

from gaussiank_sgd_amd import ops
from gaussiank_sgd_amd.utils.stats import gaussian_z

SIZES = [100, 4096 * 7 + 5, 1_000_003, 1 << 20]   # sub-tile, ragged tail, odd, aligned
N_RAGGED = 4096 * 7 + 5
INT_FIELDS = ("K", "c_gt", "overlap", "sent", "k_eff")
ENERGY_FIELDS = ("e_sel", "e_top", "e_all")
REL = 1e-5


def ratio_for(n):
    return 0.05 if n <= 10000 else 0.001


def k_for(n):
    return max(int(n * ratio_for(n)), 1)


def pair(n, seed=0, dist="normal", scale=1e-3):
    """Seeded gradient / residual pair (as tests/test_kernels_gpu.py::_pair)."""
    g = torch.Generator().manual_seed(seed)
    if dist == "normal":
        x = torch.randn(n, generator=g) * scale
        r = torch.randn(n, generator=g) * scale * 0.3
    else:
        # Student-t(2): t = z / sqrt(chi2_2 / 2), chi2_2 = -2 log U
        z = torch.randn(n, generator=g, dtype=torch.float64)
        v = -2.0 * torch.log(torch.rand(n, generator=g, dtype=torch.float64).clamp_min(1e-300))
        x = (z / torch.sqrt(v / 2.0)).float() * scale
        r = torch.zeros(n)
    return x, r


def keys_of(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF


def reference(r, record, k, k_cap):
    """fp64 reference from the compress outputs (host tensors)."""
    n = r.numel()
    sent = int(record[0])
    assert 0 <= sent <= k_cap
    idx = record[4:4 + sent].long()
    val = record[4 + k_cap:4 + k_cap + sent].view(torch.float32)
    assert float(r[idx].abs().sum()) == 0.0, "pipeline guarantee: sent entries are zero in the residual"
    acc = r.clone()
    acc[idx] = val
    k_eff = min(k, n)
    mag, _ = torch.sort(acc.abs(), descending=True)
    K = int(keys_of(mag[k_eff - 1:k_eff])[0])
    keys = keys_of(acc)
    c_gt = int((keys > K).sum())
    vk = keys_of(val) if sent else torch.zeros(0, dtype=torch.int64)
    overlap = int((vk > K).sum()) + min(int((vk == K).sum()), k_eff - c_gt)
    return {"K": K, "c_gt": c_gt, "overlap": overlap, "sent": sent, "k_eff": k_eff,
            "e_sel": float((val.double() ** 2).sum()),
            "e_top": float((mag[:k_eff].double() ** 2).sum()),
            "e_all": float((acc.double() ** 2).sum()),
            "rec_eq": int((vk == K).sum()), "acc_eq": int((keys == K).sum())}


def check(got, ref):
    for f in INT_FIELDS + ENERGY_FIELDS:
        print("%-8s got %r  reference %r" % (f, got[f], ref[f]))
    for f in INT_FIELDS:
        assert got[f] == ref[f], (f, got[f], ref[f])
    for f in ENERGY_FIELDS:
        assert abs(got[f] - ref[f]) <= REL * abs(ref[f]), (f, got[f], ref[f])
    assert got["topk_overlap"] == ref["overlap"] / ref["k_eff"]
    for f in ("energy_captured", "energy_fraction", "topk_overlap", "record_occupancy"):
        assert got[f] == got[f] and 0.0 <= got[f], (f, got[f])   # no NaN
    if ref["e_top"] == 0.0:
        assert got["energy_captured"] == 0.0


class Run:
    """compress_ then selection_quality_ on ``device``; keeps the buffers so a
    second record can go through the same ones."""

    def __init__(self, device, k_cap, n):
        self.device = torch.device(device)
        self.k_cap = k_cap
        self.bufs = ops.CompressBuffers(k_cap, self.device)
        self.out = torch.full((8,), -1.0, dtype=torch.float64, device=self.device)
        self.ws = ops.quality_workspace(self.device)
        self.r = torch.zeros(n, device=self.device)

    def __call__(self, x, r, mode, k, ec=True, loops=3, z=0.0, fixed_thr=0.0, seed=0):
        g = x.clone().to(self.device)
        self.r.copy_(r)
        ops.compress_(g, self.r, self.bufs, mode, ec=ec, zero_g=True, loops=loops, z=z, k=k, k_cap=self.k_cap,
                      seed=seed, fixed_thr=fixed_thr)
        ops.selection_quality_(self.r, self.bufs.record, k, self.k_cap, self.out, self.ws)
        got = ops.quality_fields(self.out, self.k_cap)
        ref = reference(self.r.cpu(), self.bufs.record.cpu(), k, self.k_cap)
        check(got, ref)
        return got, ref


def run(device, x, r, mode, k, k_cap, **kw):
    return Run(device, k_cap, x.numel())(x, r, mode, k, **kw)


# ---------------------------------------------------------------------------
# 1. exact top-k record
# ---------------------------------------------------------------------------
def case_topk(device, n, dist):
    x, r = pair(n, seed=n % 89 + 1, dist=dist)
    k = k_for(n)
    got, ref = run(device, x, r, ops.MODE_TOPK, k, k)
    assert got["overlap"] == got["k_eff"] and got["c_gt"] <= got["k_eff"]
    assert abs(got["e_sel"] - got["e_top"]) <= REL * got["e_top"]
    assert got["topk_overlap"] == 1.0


# ---------------------------------------------------------------------------
# 2. Gaussian-k and calibrated Gaussian-k
# ---------------------------------------------------------------------------
def case_gaussian(device, n, dist, mode):
    x, r = pair(n, seed=n % 97, dist=dist)
    k = k_for(n)
    run(device, x, r, mode, k, 2 * k, loops=3, z=gaussian_z(ratio_for(n)))


# ---------------------------------------------------------------------------
# 3. ties at the k-th magnitude
# ---------------------------------------------------------------------------
def tied_acc(n, seed=7):
    """Multiples of 2^-6 in [-1, 1]; the clipped mass at |x| = 1 is thinned to
    every 100th element (the rest moves to 63/64), so a few hundred entries lie
    above the k-th magnitude and tens of thousands share it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round((torch.randn(n, generator=g) * 0.5).clamp_(-1.0, 1.0) * 64.0) / 64.0
    top = (x.abs() == 1.0).nonzero().view(-1)
    demote = top[torch.arange(top.numel()) % 100 != 0]
    x[demote] = x[demote] * (63.0 / 64.0)
    return x


def case_ties(device, more):
    n = 1_000_003
    k = k_for(n)
    x = tied_acc(n)
    mag, _ = torch.sort(x.abs(), descending=True)
    vK = float(mag[k - 1])
    c_gt = int((x.abs() > vK).sum())
    slots = k - c_gt
    assert vK == 63.0 / 64.0 and 0 < c_gt < k and slots >= 2 and int((x.abs() == vK).sum()) > 2 * k
    # every |x| >= vK passes the threshold: far more than k_cap, so the record is
    # the exact top-k_cap -- fewer than k entries (k_cap < k) or more (k_cap = 2k)
    k_cap = 2 * k if more else c_gt + slots // 2
    got, ref = run(device, x, torch.zeros(n), ops.MODE_THRESHOLD, k, k_cap, fixed_thr=vK - 2.0 ** -7)
    assert ref["sent"] == k_cap and ref["c_gt"] == c_gt
    assert 0 < ref["rec_eq"] < ref["acc_eq"], "both sent and unsent entries carry key K"
    if more:
        assert ref["sent"] > k and ref["rec_eq"] > slots and got["overlap"] == k
    else:
        assert ref["sent"] < k and ref["rec_eq"] < slots and got["overlap"] == k_cap


# ---------------------------------------------------------------------------
# 4. keys that differ only in their low 10 bits (third radix pass)
# ---------------------------------------------------------------------------
def case_low_bits(device, mode):
    n = N_RAGGED
    g = torch.Generator().manual_seed(11)
    i = torch.arange(n)
    x = (1.0 + (i % 1024).double() * 2.0 ** -23).float()
    x = x * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    k = k_for(n)
    k_cap = k if mode == ops.MODE_TOPK else 2 * k
    got, ref = run(device, x, torch.zeros(n), mode, k, k_cap, loops=3, z=gaussian_z(ratio_for(n)))
    assert (ref["K"] >> 10) == (0x3F800000 >> 10)


# ---------------------------------------------------------------------------
# 5. degenerate inputs
# ---------------------------------------------------------------------------
def case_all_zero(device, mode):
    n = N_RAGGED
    k = k_for(n)
    k_cap = k if mode == ops.MODE_TOPK else 2 * k
    got, ref = run(device, torch.zeros(n), torch.zeros(n), mode, k, k_cap, loops=3, z=gaussian_z(ratio_for(n)))
    assert got["K"] == 0 and got["c_gt"] == 0 and got["e_top"] == 0.0 and got["e_all"] == 0.0
    assert got["overlap"] == min(ref["sent"], k)
    assert got["energy_captured"] == 0.0 and got["energy_fraction"] == 0.0


def case_few_nonzeros(device, mode):
    n = N_RAGGED
    k = k_for(n)
    x = torch.zeros(n)
    g = torch.Generator().manual_seed(3)
    pos = torch.randperm(n, generator=g)[:10]
    x[pos] = torch.randn(10, generator=g) + 2.0
    k_cap = k if mode == ops.MODE_TOPK else 2 * k
    got, ref = run(device, x, torch.zeros(n), mode, k, k_cap, fixed_thr=0.5)
    assert got["K"] == 0 and got["c_gt"] == 10 and got["k_eff"] == k > 10


def case_empty_record(device, n):
    x, r = pair(n, seed=21, dist="t")
    k = k_for(n)
    thr = float((x + r).abs().max()) * 2.0
    got, ref = run(device, x, r, ops.MODE_THRESHOLD, k, 2 * k, fixed_thr=thr)
    assert got["sent"] == 0 and got["overlap"] == 0 and got["e_sel"] == 0.0 and got["e_top"] > 0.0
    assert got["energy_captured"] == 0.0


def case_k_ge_n(device, extra):
    n = 100
    x, r = pair(n, seed=5)
    k = n + extra
    got, ref = run(device, x, r, ops.MODE_TOPK, k, k)
    assert got["k_eff"] == n and got["overlap"] == n and got["sent"] == n
    assert abs(got["e_top"] - got["e_all"]) <= REL * got["e_all"]


# ---------------------------------------------------------------------------
# 6. the same buffers (out, workspace, record) with a second record
# ---------------------------------------------------------------------------
def case_second_call(device):
    n = N_RAGGED
    k = k_for(n)
    rn = Run(device, 2 * k, n)
    x, r = pair(n, seed=41, dist="t")
    first, _ = rn(x, r, ops.MODE_GAUSSIAN, k, loops=3, z=gaussian_z(ratio_for(n)))
    x2, r2 = pair(n, seed=42, dist="normal", scale=3e-2)
    second, ref2 = rn(x2, r2, ops.MODE_TOPK, k)
    assert second["K"] != first["K"] and not math.isclose(second["e_all"], first["e_all"], rel_tol=0.5)
    # and back: the first inputs again give the first result (integer fields exactly)
    again, _ = rn(x, r, ops.MODE_GAUSSIAN, k, loops=3, z=gaussian_z(ratio_for(n)))
    assert all(again[f] == first[f] for f in INT_FIELDS)


# ---------------------------------------------------------------------------
# 7. DistributedOptimizer sampling
# ---------------------------------------------------------------------------
def optimizer_run(device, comp, every, steps=6):
    """One process, fcn5net: (rows, weights, residuals, records) after ``steps`` steps."""
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    torch.manual_seed(0)
    comm.init()
    t = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", batch_size=32, lr=0.05, device=device, learnable_data=True)
    opt = DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(), compression=compressors[comp],
                               is_sparse=True, density=0.01, compress_single_rank=True, density_warmup=False,
                               threshold=10_000, selection_quality_every=every)
    t.update_optimizer(opt)
    for _ in range(steps):
        opt.zero_grad()
        t.train(1)
        t.update_model()
    rows = opt.collect_selection_quality()
    arena = opt.arena
    state = (arena.weights.detach().cpu().clone(), arena.residuals.detach().cpu().clone(),
             [b.bufs.record.detach().cpu().clone() for b in arena.buckets])
    return rows, state, len(arena.buckets), opt


def check_rows(rows, nbuckets, every, steps, comp):
    assert nbuckets > 1
    expect = [(it, b) for it in range(0, steps, every) for b in range(nbuckets)]
    assert sorted((r["iter"], r["bucket"]) for r in rows) == expect
    for r in rows:
        assert 0 < r["k_eff"] and 0 <= r["overlap"] <= r["k_eff"] and r["sent"] > 0
        # e_top <= e_all; a record with more than k_eff entries may capture more than e_top
        assert 0.0 < r["energy_fraction"] <= min(r["energy_captured"], 1.0) * (1.0 + REL)
        if comp == "topk":
            assert r["topk_overlap"] == 1.0 and abs(r["energy_captured"] - 1.0) <= REL, r


def states_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2]) and \
        all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
