"""FP8 quantisers, the K = 128 MFMA GEMM and the FastLinear path on them (ops/fp8.py,
csrc/kernels/fp8.hip) against torch float8 casts and fp64 products of the dequantised operands."""
import math

import pytest
import torch
import torch.nn.functional as F

from gaussiank_sgd_amd.ops import fp8, linear
from gaussiank_sgd_amd.ops.linear import FastLinear

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _data(R, C, seed=0, outlier=37.0):
    """Seeded normal data, another magnitude per row and per column, one outlier that sets amax."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=g) * torch.linspace(0.5, 2, R)[:, None] * torch.linspace(0.25, 4, C)[None, :]
    x[R // 2, C // 3] = outlier
    return x


def _ref_quant(x, fmt):
    """(q, e) by the rule of ops/fp8.py, on the CPU: e by search in exact double arithmetic."""
    x = x.detach().float().cpu()
    amax, fmax = float(x.abs().max()), fp8.FMAX[fmt]
    e = 0
    if amax > 0:
        e = math.floor(math.log2(fmax / amax))
        e += (amax * 2.0 ** (e + 1) <= fmax) - (amax * 2.0 ** e > fmax)
    e = max(-64, min(64, e))
    return (x * 2.0 ** e).to(fp8.DTYPE[fmt]), e


def _bits(q):
    return q.view(torch.uint8).cpu()


def _case(name, fmt):
    if isinstance(name, tuple):
        return _data(*name)
    if name == "zero":
        return torch.zeros(3, 384)
    if name == "pow2":      # amax exactly a power of two times FMAX
        return _data(3, 384, outlier=fp8.FMAX[fmt] / 8)
    x = _data(3, 384)       # "tiny": rows below the smallest subnormal of the format, and around it, after scaling
    x[0] *= 1e-8
    x[2] *= 1e-4
    return x


@pytest.mark.parametrize("case", [(1, 128), (3, 384), (257, 1024), "zero", "pow2", "tiny"], ids=str)
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_quantisers_bit_for_bit(cuda, fmt, dtype, case):
    x = _case(case, fmt).to(dtype)
    ref, e = _ref_quant(x, fmt)
    q, scale = fp8.quantize(x.to(cuda), fmt)
    assert q.dtype == fp8.DTYPE[fmt] and float(scale) == 2.0 ** -e
    assert torch.equal(_bits(q), _bits(ref))
    if fmt == "e4m3":
        w8, w8t, sw = fp8.quantize_weight(x.to(cuda))
        assert float(sw) == 2.0 ** -e
        assert torch.equal(_bits(w8), _bits(ref)) and torch.equal(_bits(w8t), _bits(ref).t())


def _tol(a8, b8, s, bias, ref, K):
    """2 E + 2^-8 |ref|, E = K 2^-23 ((|A8| |B8|^T) s + |bias|): products of two 8-bit floats are exact in
    fp32, E bounds K fp32 additions to first order, 2^-8 covers the rounding to bf16."""
    E = K * 2.0 ** -23 * ((a8.abs() @ b8.abs().t()) * s + (bias.abs() if bias is not None else 0.0))
    return 2 * E + 2.0 ** -8 * ref.abs()


# one tile and one K step (pins the operand layout); an odd number of K steps through the double buffer;
# a row tail and several tiles; a single row
@pytest.mark.parametrize("M,N,K", [(16, 128, 128), (128, 128, 384), (200, 256, 256), (1, 128, 1024)])
@pytest.mark.parametrize("afmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_gemm_against_fp64(cuda, M, N, K, afmt, with_bias):
    a8, sa = fp8.quantize(_data(M, K, 1).to(BF16).to(cuda), afmt)
    b8, sb = fp8.quantize(_data(N, K, 2, outlier=-5.0).to(BF16).to(cuda), "e4m3")
    bias = 3 * torch.randn(N, generator=torch.Generator().manual_seed(3)) if with_bias else None
    out = fp8.gemm_nt(a8, sa, b8, sb, bias.to(cuda) if with_bias else None)
    assert out.dtype == BF16 and out.shape == (M, N)
    a, b, s = a8.cpu().double(), b8.cpu().double(), float(sa) * float(sb)
    ref = (a @ b.t()) * s + (bias.double() if with_bias else 0.0)
    err = (out.cpu().double() - ref).abs()
    tol = _tol(a, b, s, bias.double() if with_bias else None, ref, K)
    print("max |out - ref| / tol = %.3f" % float((err / tol.clamp_min(1e-300)).max()))
    assert bool((err <= tol).all())


@pytest.fixture
def fp8_on():
    linear.set_fp8(True)
    yield
    linear.set_fp8(False)


def _run(lin, x, dy, act):
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        y = lin(x, act=act)
    dx, dw, db = torch.autograd.grad(y, (x, lin.weight, lin.bias), dy)
    return y, dx, dw, db


@pytest.mark.parametrize("tokens,fin,fout", [(256, 128, 384), (200, 256, 128)])
@pytest.mark.parametrize("act", [None, "gelu"])
def test_fastlinear_end_to_end(cuda, fp8_on, tokens, fin, fout, act):
    torch.manual_seed(0)
    lin = FastLinear(fin, fout).to(cuda)
    with torch.no_grad():
        lin.bias.normal_()
    x, dy = _data(tokens, fin, 4).to(BF16).to(cuda), _data(tokens, fout, 5, outlier=-3.0).to(BF16).to(cuda)
    y, dx, dw, db = _run(lin, x, dy, act)
    # the emulation: quantise, fp64 matmul, bias, bf16
    x8, ex = _ref_quant(x, "e4m3")
    w8, ew = _ref_quant(lin.weight.to(BF16), "e4m3")
    bias = lin.bias.detach().cpu().double()
    pre = (x8.double() @ w8.double().t()) * 2.0 ** -(ex + ew) + bias
    tol = _tol(x8.double(), w8.double(), 2.0 ** -(ex + ew), bias, pre, fin)
    dpre = dy
    if act == "gelu":
        # gelu' <= 1.13, then one more rounding to bf16; the backward's dpre is the (separately tested)
        # GELU-backward pass on the kernel's own pre-activation, which the act=None run returns
        ref_y = F.gelu(pre)
        tol = 1.13 * tol + 2.0 ** -8 * ref_y.abs()
        dpre = linear.gelu_backward_(dy, _run(lin, x, dy, None)[0].detach())
    else:
        ref_y = pre
    assert bool(((y.detach().cpu().double() - ref_y).abs() <= tol).all())
    d8, ed = _ref_quant(dpre, "e5m2")
    ref_dx = (d8.double() @ w8.double()) * 2.0 ** -(ed + ew)
    tol_dx = _tol(d8.double(), w8.double().t(), 2.0 ** -(ed + ew), None, ref_dx, fout)
    assert bool(((dx.cpu().double() - ref_dx).abs() <= tol_dx).all())
    if act is None:
        # weight and bias gradients: the same bf16 kernels on the same inputs as with fp8 off
        linear.set_fp8(False)
        _, _, dw0, db0 = _run(lin, x, dy, None)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)


@pytest.mark.parametrize("fin,opt_out", [(128, True), (192, False)])
def test_opt_out_and_unsupported_width_take_the_bf16_path(cuda, fp8_on, fin, opt_out):
    torch.manual_seed(0)
    lin = FastLinear(fin, 128).to(cuda)
    if opt_out:
        lin.fp8 = False
    x = _data(64, fin, 6).to(BF16).to(cuda)
    with torch.autocast("cuda", dtype=BF16):
        y = lin(x)
        linear.set_fp8(False)
        lin.fp8 = None
        assert torch.equal(y, lin(x))


def test_forward_backward_in_a_graph_reads_nothing_on_the_host(cuda, fp8_on):
    torch.manual_seed(0)
    lin = FastLinear(128, 384).to(cuda)
    xs, dys = torch.zeros(256, 128, dtype=BF16, device=cuda), torch.zeros(256, 384, dtype=BF16, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up off the capture
        _run(lin, xs.normal_(), dys.normal_(), "gelu")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    xg = xs.requires_grad_(True)
    with torch.cuda.graph(graph):
        with torch.autocast("cuda", dtype=BF16):
            yg = lin(xg, act="gelu")
        (dxg,) = torch.autograd.grad(yg, xg, dys)   # the 8-bit path; the grad-weight is the bf16 kernel as before
    for seed in (7, 8, 9):   # several replays on new data against the eager call
        x, dy = _data(256, 128, seed).to(BF16).to(cuda), _data(256, 384, seed + 10, outlier=-2.0).to(BF16).to(cuda)
        with torch.no_grad():
            xs.copy_(x)
            dys.copy_(dy)
        graph.replay()
        y, dx, _, _ = _run(lin, x, dy, "gelu")
        assert torch.equal(yg, y) and torch.equal(dxg, dx)
