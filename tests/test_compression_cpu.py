"""CPU tests: the torch mirror of the fused pipeline vs the reference-semantics
oracles, record layout, conservation, and the compressor registry API."""
import math

import pytest
import torch

from gaussiank_sgd_amd import ops
from gaussiank_sgd_amd.compression import compressors, reference
from gaussiank_sgd_amd.utils.stats import gaussian_z, gen_threshold_from_normal_distribution, norm_ppf


def _mirror(x, r, mode, k, k_cap, ec=True, loops=3, z=0.0, seed=0, fixed=0.0):
    b = ops.CompressBuffers(k_cap, "cpu")
    g, rr = x.clone(), r.clone()
    ops.compress_(g, rr, b, mode, ec=ec, zero_g=True, loops=loops, z=z, k=k, k_cap=k_cap, seed=seed,
                  fixed_thr=fixed)
    rec = b.record
    sent = int(rec[0])
    return g, rr, rec, rec[4:4 + sent].long(), rec[4 + k_cap:4 + k_cap + sent].view(torch.float32), b


def test_norm_ppf_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    for p in [1e-9, 1e-4, 0.0005, 0.01, 0.3, 0.5, 0.9, 0.999]:
        assert abs(norm_ppf(p) - float(stats.norm.ppf(p))) < 1e-12 * max(1, abs(norm_ppf(p))) + 1e-14


def test_gaussian_threshold_selfcheck():
    # reference compression.py:757-777: recover a 3-sigma threshold from its p-value
    g = torch.Generator().manual_seed(0)
    d = torch.randn(200_000, generator=g, dtype=torch.float64) * 0.5
    std, mean = float(d.std()), float(d.mean())
    thres = 3 * std
    pvalue = 1 - float((d.abs() >= thres).sum()) / d.numel()
    _, right = gen_threshold_from_normal_distribution(pvalue, mean, std)
    assert abs(right - thres) / thres < 0.03


@pytest.mark.parametrize("loops,ec", [(3, True), (5, False)])
@pytest.mark.parametrize("dist", ["normal", "t"])
def test_gaussian_mirror_equals_reference(loops, ec, dist):
    g = torch.Generator().manual_seed(1)
    n = 100_000
    if dist == "normal":
        x = torch.randn(n, generator=g) * 1e-2
    else:
        x = torch.distributions.StudentT(2.0).sample((n,)) * 1e-2
    r = torch.randn(n, generator=g) * 1e-3
    ratio = 0.001
    k = int(n * ratio)
    _, rr, rec, idx, val, b = _mirror(x, r, ops.MODE_GAUSSIAN, k, n, ec, loops, gaussian_z(ratio))
    st = b.stats
    acc, ridx, rval, rres = reference.gaussian(x, r, ratio, loops=loops, ec=ec,
                                               stats=(float(st[0]), float(st[1])))
    assert torch.equal(idx, ridx)
    assert torch.equal(val, rval)
    assert torch.equal(rr, rres)


def test_topk_mirror_equals_exact_and_torch_topk_set():
    g = torch.Generator().manual_seed(2)
    n = 50_000
    x = torch.randn(n, generator=g)
    r = torch.zeros(n)
    k = 50
    _, rr, rec, idx, val, _ = _mirror(x, r, ops.MODE_TOPK, k, k)
    _, tidx = torch.topk(x.abs(), k)
    assert set(idx.tolist()) == set(tidx.tolist())
    assert bool((idx[1:] > idx[:-1]).all())


@pytest.mark.parametrize("mode", ["redsync", "redsynctrim"])
def test_redsync_mirror_vs_reference(mode):
    g = torch.Generator().manual_seed(3)
    n = 80_000
    x = torch.distributions.StudentT(3.0).sample((n,))
    r = torch.zeros(n)
    k = 80
    m = ops.MODE_REDSYNC if mode == "redsync" else ops.MODE_REDSYNCTRIM
    _, rr, rec, idx, val, _ = _mirror(x, r, m, k, n)
    fn = reference.redsync if mode == "redsync" else reference.redsynctrim
    _, ridx, _, _ = fn(x, r, 0.001)
    # thresholds are computed from fp32 mean/max that can differ by 1 ulp: allow +-1 element
    assert abs(idx.numel() - ridx.numel()) <= 1
    assert len(set(idx.tolist()) ^ set(ridx.tolist())) <= 1


def test_conservation_and_cap():
    g = torch.Generator().manual_seed(4)
    n = 10_000
    x = torch.randn(n, generator=g)
    r = torch.randn(n, generator=g) * 0.1
    k_cap = 7
    _, rr, rec, idx, val, _ = _mirror(x, r, ops.MODE_THRESHOLD, 5, k_cap, fixed=1.0)
    acc = x + r
    assert int(rec[0]) == k_cap and int(rec[1]) == int((acc.abs() > 1.0).sum())
    rebuilt = rr.clone()
    rebuilt[idx] += val
    assert torch.equal(rebuilt, acc)
    # overflow is cut by magnitude (exact top-k_cap), not by index order
    assert int(rec[2]) == ops.OVERFLOW_EXACT
    assert set(idx.tolist()) == set(torch.topk(acc.abs(), k_cap).indices.tolist())


@pytest.mark.parametrize("k_cap_mult", [4.0 / 3.0, 1.0, 3.0])
def test_gaussian_overflow_sends_largest(k_cap_mult):
    """Heavy-tailed bucket: the reference tree stops far above k (the VGG /
    multi-bucket case).  The record must hold <= k_cap entries that are the
    LARGEST |x| (every sent magnitude >= every unsent one), the header keeps
    the reference rule's count, and nothing is lost (conservation)."""
    g = torch.Generator().manual_seed(11)
    n = 200_000
    x = torch.randn(n, generator=g) * 1e-4
    x[torch.randperm(n, generator=g)[: n // 2]] = 0.0      # heavy-zero gradient (ReLU nets)
    hot = torch.randperm(n, generator=g)[: n // 50]         # 2% outliers dominate sigma
    x[hot] = (1.0 + torch.rand(hot.numel(), generator=g)) * torch.sign(torch.randn(hot.numel(), generator=g))
    r = torch.zeros(n)
    ratio = 0.001
    k = int(n * ratio)
    k_cap = max(1, math.ceil(k * k_cap_mult))
    _, rr, rec, idx, val, _ = _mirror(x, r, ops.MODE_GAUSSIAN, k, k_cap, z=gaussian_z(ratio))
    acc = x + r
    ref_total = int(reference.gaussian(x, r, ratio, loops=3, ec=True)[1].numel())
    assert int(rec[1]) == ref_total and ref_total > k_cap        # the reference overflows
    sent = int(rec[0])
    assert 0 < sent <= k_cap
    unsent = torch.ones(n, dtype=torch.bool)
    unsent[idx] = False
    assert float(val.abs().min()) >= float(acc.abs()[unsent].max())
    assert bool((idx[1:] > idx[:-1]).all())
    rebuilt = rr.clone()
    rebuilt[idx] += val
    assert torch.equal(rebuilt, acc)


def test_dgc_mirror_semantics():
    g = torch.Generator().manual_seed(5)
    n = 200_000
    x = torch.randn(n, generator=g)
    r = torch.zeros(n)
    k = 200
    _, rr, rec, idx, val, _ = _mirror(x, r, ops.MODE_DGC, k, 4 * k, seed=42)
    total = int(rec[1])
    assert 0 < total <= math.ceil(4 * k / 3) or total == k


def test_scatter_cpu_unequal_counts():
    P, k_cap, n = 3, 10, 50
    recs = torch.zeros(P, 4 + 2 * k_cap, dtype=torch.int32)
    per = []
    for p in range(P):
        cnt = 3 + 2 * p
        idx = torch.arange(cnt) * 2
        val = torch.full((cnt,), float(p + 1))
        recs[p, 0] = cnt
        recs[p, 4:4 + cnt] = idx.int()
        recs[p, 4 + k_cap:4 + k_cap + cnt] = val.view(torch.int32)
        per.append((idx, val))
    dst = torch.zeros(n)
    ops.scatter_add_records_(dst, recs, P, k_cap, 1.0 / P)
    assert torch.allclose(dst, reference.sparse_aggregate(n, per, P))


def test_registry_api_compat():
    for name in ["topk", "topk2", "gaussian", "gaussian2", "randomk", "randomkec", "dgcsampling", "redsync",
                 "redsynctrim", "topk_legacy"]:
        c = compressors[name]
        c.clear()
        t = torch.randn(5000)
        orig = t.clone()
        out, idx, vals = c.compress(t, "layer", ratio=0.01)
        assert out is t
        assert idx.dtype == torch.int64 and vals.numel() == idx.numel() > 0
        assert torch.equal(vals, t[idx])
        if getattr(c, "ec", False) or name == "topk_legacy":
            assert torch.equal(t, orig)  # first call: residual was zero
        res = c.residuals["layer"]
        assert float(res[idx].abs().sum()) == 0.0
    t = torch.randn(100)
    out, ctx, means = compressors["bucket"].compress(t.clone(), "b")
    assert ctx is None and means.numel() == 2
    out, ctx, sel = compressors["none"].compress(t, "n")
    assert sel is t


def test_topk_legacy_is_uniform_101():
    t = torch.randn(20_000)
    _, idx, _, _ = reference.uniform_abs_topk(t, None, 0.001, ec=False)
    sorted_index = t.abs().argsort()
    assert torch.equal(idx, sorted_index[::101][-20:])


def _bin_loop_bucketized(tensor, k):
    """Literal per-bin statement of the reference rule (compression.py:60-93),
    independent of the vectorised oracle."""
    import torch
    n = tensor.numel()
    si = torch.argsort(torch.abs(tensor), descending=True, stable=True)
    vals = (tensor[si] * 100).int()
    _, counts = torch.unique(vals, sorted=True, return_counts=True)
    take, rest, start = [], [], 0
    for c in counts.tolist():
        e = c if c == 1 else round((c * k) / n)
        take += si[start:start + e].tolist()
        rest += si[start + e:start + c].tolist()
        start += c
    if len(take) < k:
        take += rest[:k - len(take)]
    return take[:k]


def test_bucketized_topk_matches_bin_loop_and_quirk():
    import torch
    from gaussiank_sgd_amd.compression import compressors, reference
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5000, generator=g) * 0.05
    for ratio in (0.001, 0.01, 0.05):
        k = max(int(x.numel() * ratio), 1)
        acc, idx, vals, res = reference.bucketized_topk(x, None, ratio, ec=False)
        assert idx.tolist() == _bin_loop_bucketized(x, k)
        assert idx.numel() == k and torch.equal(vals, x[idx])
        assert torch.equal(res[idx], torch.zeros(k)) and torch.equal(acc, x)
    # the quirk: the selection is NOT the top-k by magnitude
    k = 50
    _, idx, _, _ = reference.bucketized_topk(x, None, k / x.numel(), ec=False)
    top = set(torch.topk(x.abs(), k).indices.tolist())
    assert len(top & set(idx.tolist())) < k
    # registry: EC compressor with the reference's (tensor, indexes, values) API
    comp = compressors["bucketized_topk"]
    comp.clear()
    t = x.clone()
    out, i2, v2 = comp.compress(t, name="b", ratio=0.01)
    assert out is t and i2.numel() == 50 and torch.equal(comp.residuals["b"][i2], torch.zeros(50))
    assert torch.allclose(comp.residuals["b"] + torch.zeros_like(x).index_put_((i2,), v2), x)


def test_bucketized_topk_against_reference_source():
    """The indices the reference's own bucketized_topk returned on a fixed
    tensor with distinct magnitudes (recorded in tests/golden/bucketized_topk.npz:
    the input ``x`` and ``idx_k<k>`` per k) are reproduced exactly."""
    import os
    import numpy as np
    import torch
    from gaussiank_sgd_amd.compression import reference
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bucketized_topk.npz"))
    x = torch.from_numpy(gold["x"])
    assert x.dtype == torch.float32 and x.numel() == 4000
    for ratio in (0.002, 0.01, 0.04):
        k = max(int(x.numel() * ratio), 1)
        ref_idx = gold["idx_k%d" % k]
        assert ref_idx.size == k
        _, idx, _, _ = reference.bucketized_topk(x, None, ratio, ec=False)
        assert idx.tolist() == ref_idx.tolist()


def test_gaussian_overflow_extension_node():
    """Power-law tail: the reference walk (t0, 1.5 t0, 2.25 t0) still passes
    more than k_cap entries; one of the overflow-extension thresholds
    (2.25 t0 * 1.25^j, ladder slots 6..15) lands in [2k/3, k_cap] and is chosen
    -- a magnitude-correct selection from the same count pass, no exact
    fallback.  The header keeps the reference rule's count."""
    g = torch.Generator().manual_seed(21)
    n = 400_000
    u = torch.rand(n, generator=g).clamp_min(1e-12)
    x = (u ** (-1.0 / 2.5) - 1.0) * 1e-3 * torch.sign(torch.randn(n, generator=g))   # Pareto(2.5) tail
    r = torch.zeros(n)
    ratio = 0.001
    k = int(n * ratio)
    k_cap = math.ceil(4 * k / 3)
    z = gaussian_z(ratio)
    _, rr, rec, idx, val, b = _mirror(x, r, ops.MODE_GAUSSIAN, k, k_cap, z=z)
    ref_total = int(reference.gaussian(x, r, ratio, loops=3, ec=True)[1].numel())
    assert ref_total > k_cap and int(rec[1]) == ref_total
    chosen = int(rec[2])
    assert 6 <= chosen < ops.MAX_CAND, chosen
    sent = int(rec[0])
    assert 2 * k <= 3 * sent <= 3 * k_cap
    acc = x + r
    thr = float(rec[3:4].view(torch.float32))
    assert torch.equal(idx, (acc.abs() > thr).nonzero().view(-1))
    # the threshold is the walk's top node times 1.25^(chosen - 5)
    mean, std = float(acc.double().mean()), float(acc.double().std())
    t = (mean + z * std) * 2.25 * 1.25 ** (chosen - 5)
    assert abs(thr - t) <= 1e-6 * t
    rebuilt = rr.clone()
    rebuilt[idx] += val
    assert torch.equal(rebuilt, acc)
