"""Backward of a stride-2 transition bottleneck (ops/bn.py ``BnLink.dy2c``):
the 1x1 stride-2 downsample's grad-input stays compact (``conv1x1._dgrad_ds``,
a quarter-M row GEMM) and conv1's grad-input adds it at the even pixels in its
BN-backward epilogue (``conv1x1._dgrad_bn_ds``, gemm_nt_x62_kernel), so the
block input's BN needs no reduction pass of its own.

Tolerances are the project's: the fp32 bf16x6 epilogue tests'
(tests/test_gemm_x6_gpu.py ``_tol`` and its partial-sum ``allclose``) at kernel
level, the "fused no worse than unfused" rule of tests/test_bnlink_gpu.py at
network level."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CL = torch.channels_last
X6 = 100000
# every register-staged tile, B split in the kernel (2) and pre-split (3)
X62_CFGS = [f * X6 + t for f in (2, 3) for t in range(1, 8)]


@pytest.fixture(scope="module")
def g():
    from gaussiank_sgd_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load(), ops._load_error
    return torch.ops.gksgd


def _tol(ref_abs):
    return 2e-6 * ref_abs.max().item() + 1e-6


def _scatter(d2c, Nb, H, W):
    """[Nb * OH * OW, C] compact rows -> [Nb * H * W, C] rows, zeros off the even pixels."""
    OH, OW = (H + 1) // 2, (W + 1) // 2
    C = d2c.shape[1]
    full = torch.zeros(Nb, H, W, C, dtype=d2c.dtype, device=d2c.device)
    full[:, ::2, ::2] = d2c.view(Nb, OH, OW, C)
    return full.view(Nb * H * W, C)


# (3, 7, 5): OH = 4, OW = 3, an odd last row and column, M = 105 is no multiple of a tile;
# (5, 9, 7) with 256 columns: several M tiles per block column and the 256-wide tiles themselves
@pytest.mark.parametrize("Nb,H,W,C,K", [(2, 8, 8, 128, 64), (3, 7, 5, 128, 64), (5, 9, 7, 256, 64)])
@pytest.mark.parametrize("cfg", X62_CFGS)
def test_compact_dy2_epilogue(g, cfg, Nb, H, W, C, K):
    """dz = mask ? (A B^T + scatter(dy2c)) : 0 with the partials sum(dz), sum(dz * h)."""
    torch.manual_seed(cfg + H * W)
    M, OH, OW = Nb * H * W, (H + 1) // 2, (W + 1) // 2
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(C, K, device="cuda") * K ** -0.5
    h = torch.randn(M, C, device="cuda")
    d2c = torch.randn(Nb * OH * OW, C, device="cuda")
    keep = torch.rand(M, C // 4, 4, device="cuda") > 0.3
    mask = (keep.to(torch.uint8) * torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device="cuda")).sum(-1).to(torch.uint8)
    out = torch.full((M, C), float("nan"), device="cuda")
    st = torch.full((2, min(1280, (M + 63) // 64), C), float("nan"), device="cuda")
    rows = g.gemm_nt(A, B, out, cfg, 0, st, None, h, d2c, mask, bn_dy2_geo=[H, W, OH, OW])
    dx = A.double() @ B.double().t() + _scatter(d2c.double(), Nb, H, W)
    dz = torch.where(keep.reshape(M, C), dx, torch.zeros_like(dx))
    err = (out.double() - dz).abs().max().item()
    print("cfg %d geo %s: max err %.3g" % (cfg, (Nb, H, W), err))
    assert err <= _tol(A.double().abs() @ B.double().abs().t() + 4), err
    s = st[:, :rows].double().sum(1)
    assert torch.allclose(s[0], dz.sum(0), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[1], (dz * h.double()).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("cfg", [3, X6 + 3, 1001, 2 * X6 + 20001])
def test_compact_dy2_refused_elsewhere(g, cfg):
    """Only one register-staged row GEMM reads a compact dy2: the fp32-MFMA and
    LDS-DMA bf16x6 families and split-K refuse it instead of misreading it."""
    Nb, H, W, C, K = 2, 8, 8, 128, 128
    M = Nb * H * W
    A, B, h = torch.randn(M, K, device="cuda"), torch.randn(C, K, device="cuda"), torch.randn(M, C, device="cuda")
    d2c = torch.randn(Nb * 16, C, device="cuda")
    out = torch.empty(M, C, device="cuda")
    st = torch.empty(2, 2, C, device="cuda")
    with pytest.raises(RuntimeError):
        g.gemm_nt(A, B, out, cfg, 0, st, None, h, d2c, None, bn_dy2_geo=[H, W, 4, 4])


@pytest.mark.parametrize("Nb,H,W", [(2, 8, 8), (3, 7, 5)])
def test_compact_ds_dgrad(g, monkeypatch, Nb, H, W):
    """The compact 1x1 stride-2 grad-input is the even-pixel subset of what
    conv_dgrad_s2 stores; every other pixel of that is an exact zero."""
    from gaussiank_sgd_amd.ops import autotune, conv1x1
    monkeypatch.setattr(autotune, "_TUNE", False)
    monkeypatch.setattr(autotune, "_choices", {})
    torch.manual_seed(H)
    C, K = 128, 64
    OH, OW = (H + 1) // 2, (W + 1) // 2
    dy = torch.randn(Nb, K, OH, OW, device="cuda").contiguous(memory_format=CL)
    w = (torch.randn(K, C, 1, 1, device="cuda") * K ** -0.5).contiguous(memory_format=CL)
    full = torch.full((Nb, C, H, W), float("nan"), device="cuda").contiguous(memory_format=CL)
    g.conv_dgrad_s2(dy, w, full, torch.zeros(256, dtype=torch.bfloat16, device="cuda"), 0, 0)
    dxc = conv1x1._dgrad_ds(dy, w, (Nb, C, H, W))
    assert dxc.shape == (Nb * OH * OW, C)
    sub = full[:, :, ::2, ::2].permute(0, 2, 3, 1).reshape(Nb * OH * OW, C)
    rows_dy = dy.permute(0, 2, 3, 1).reshape(-1, K).double()
    bound = rows_dy.abs() @ w.reshape(K, C).double().abs()
    err = (dxc.double() - sub.double()).abs().max().item()
    print("geo %s: compact vs conv_dgrad_s2 %.3g" % ((Nb, H, W), err))
    assert err <= _tol(bound), err
    assert (dxc.double() - rows_dy @ w.reshape(K, C).double()).abs().max().item() <= _tol(bound)
    rest = full.clone()
    rest[:, :, ::2, ::2] = 0
    assert torch.equal(rest, torch.zeros_like(rest))


class _TwoBlocks(nn.Module):
    """A stride-1 bottleneck, then a stride-2 transition bottleneck with a ConvBN
    downsample, wired as models/resnet_imagenet.py wires a ResNet."""

    def __init__(self):
        super().__init__()
        from gaussiank_sgd_amd.models.resnet_imagenet import Bottleneck, ConvBN, conv1x1
        from gaussiank_sgd_amd.ops.bn import BNAct
        self.b1 = Bottleneck(64, 64, 1, ConvBN(conv1x1(64, 256, 1), BNAct(256)))
        self.b2 = Bottleneck(256, 64, 2, ConvBN(conv1x1(256, 256, 2), BNAct(256)))
        self.b1.bn3.twin = True
        for b in (self.b1, self.b2):
            b.bn1.bwd_link = b.bn2.bwd_link = True
        self.b1.bn3.bwd_link = True

    def forward(self, x):
        return self.b2(self.b1(x))


def _grads(model, x):
    model.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    model(x).square().mean().backward()
    out = {n: p.grad.detach().double().clone() for n, p in model.named_parameters()}
    out["input"] = x.grad.detach().double().clone()
    return out


class _Spy:
    """torch.ops.gksgd with the data pointers of every bn_act_backward's BN input recorded."""

    def __init__(self, ops, seen):
        self._ops, self._seen = ops, seen

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name != "bn_act_backward":
            return fn

        def spy(dy, mask, x, *a, **k):
            self._seen.append(x.data_ptr())
            return fn(dy, mask, x, *a, **k)
        return spy


@pytest.fixture(scope="module")
def two_blocks(g):
    torch.manual_seed(0)
    m = _TwoBlocks().cuda().to(memory_format=CL).train()
    x = torch.randn(2, 64, 8, 8, device="cuda").contiguous(memory_format=CL)
    # fp64 on the CPU: plain torch ops throughout
    ref = {n: v.cuda() for n, v in _grads(copy.deepcopy(m).cpu().double(), x.cpu().double()).items()}
    return m, x, ref


def _rel(got, ref):
    return {n: float((got[n] - ref[n]).norm() / (ref[n].norm() + 1e-30)) for n in ref}


def test_two_block_net_fused_fallback_off(two_blocks, monkeypatch):
    """Parameter and input gradients with the fusion on, off and on the forced
    fallback (conv1 cannot fuse: the BN backward scatters the compact gradient),
    each against fp64: neither new path is worse than the unfused one."""
    from gaussiank_sgd_amd.ops import autotune, bn, conv1x1
    m, x, ref = two_blocks
    monkeypatch.setattr(autotune, "_TUNE", False)
    monkeypatch.setattr(autotune, "_choices", {})
    calls, seen, bn3_in = [], [], []
    for name in ("_dgrad_ds", "_dgrad_bn_ds"):
        def counting(*a, _f=getattr(conv1x1, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(conv1x1, name, counting)
    real_ops = bn._ops()
    monkeypatch.setattr(bn, "_ops", lambda: _Spy(real_ops, seen))
    hook = m.b1.bn3.register_forward_pre_hook(lambda mod, args: bn3_in.append(args[0].data_ptr()))
    try:
        monkeypatch.setenv("GKSGD_BN_LINK_DS", "0")
        e_off = _rel(_grads(m, x), ref)
        assert not calls
        assert bn3_in[-1] in seen, "unfused: the block output's BN runs its own reduction"
        monkeypatch.setenv("GKSGD_BN_LINK_DS", "1")
        del seen[:]
        e_on = _rel(_grads(m, x), ref)
        assert calls == ["_dgrad_ds", "_dgrad_bn_ds"], calls
        assert bn3_in[-1] not in seen, "the twin bn_act_backward ran beside the fused grad-input"
        del calls[:], seen[:]
        monkeypatch.setattr(conv1x1, "_ds_fusable", lambda *a, **k: False)
        e_fb = _rel(_grads(m, x), ref)
        assert calls == ["_dgrad_ds"], calls
        assert bn3_in[-1] in seen
    finally:
        hook.remove()
    worse = []
    for n in ref:
        print("%-28s off %.3g on %.3g fallback %.3g" % (n, e_off[n], e_on[n], e_fb[n]))
        for e in (e_on[n], e_fb[n]):
            if e > 1.5 * e_off[n] + 2e-3:
                worse.append((n, e, e_off[n]))
    assert not worse, worse


def test_two_block_net_graph_replay(two_blocks, monkeypatch):
    """The fused path captured in a HIP graph and replayed gives the eager step's
    gradients (the reference-batch phases replay their steps as graphs)."""
    from gaussiank_sgd_amd.ops import autotune, conv1x1
    m, x, ref = two_blocks
    monkeypatch.setattr(autotune, "_TUNE", False)
    monkeypatch.setattr(autotune, "_choices", {})
    calls = []
    orig = conv1x1._dgrad_bn_ds
    monkeypatch.setattr(conv1x1, "_dgrad_bn_ds", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e_eager = _rel(_grads(m, x), ref)       # also settles every kernel choice before the capture
    torch.cuda.current_stream().wait_stream(side)
    assert calls == [1]
    m.zero_grad(set_to_none=True)
    xg = x.detach().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(xg).square().mean().backward()
    assert calls == [1, 1]
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().double() for n, p in m.named_parameters()}
    got["input"] = xg.grad.detach().double()
    e_graph = _rel(got, ref)
    worse = [(n, e_graph[n], e_eager[n]) for n in ref if e_graph[n] > 1.5 * e_eager[n] + 2e-3]
    assert not worse, worse
