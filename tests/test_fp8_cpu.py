"""The FP8 scale rule, the CPU emulation of ops/fp8.py and the --fp8-linear flag."""
import math

import pytest
import torch

from gaussiank_sgd_amd.ops import fp8

_UP = float("inf")


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("e", [-3, 0, 5])
def test_scale_exponent_at_and_above_the_boundary(fmt, e):
    at = torch.tensor([fp8.FMAX[fmt] * 2.0 ** -e], dtype=torch.float32)   # amax * 2^e == FMAX exactly
    above = torch.nextafter(at, torch.tensor([_UP]))
    assert int(fp8.scale_exponent(at, fmt)) == e
    assert int(fp8.scale_exponent(above, fmt)) == e - 1


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("amax,want", [(0.0, 0), (1e-30, 64), (1e-45, 64), (1e30, -64), (1.0, None)])
def test_scale_exponent_zero_and_clamp(fmt, amax, want):
    if want is None:
        want = math.floor(math.log2(fp8.FMAX[fmt]))
    assert int(fp8.scale_exponent(torch.tensor([amax], dtype=torch.float32), fmt)) == want


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_emulated_quantize_and_gemm(fmt):
    torch.manual_seed(0)
    x = torch.randn(5, 128) * torch.linspace(0.25, 4, 128)
    x[2, 7] = 37.0
    w = torch.randn(128, 128).to(torch.bfloat16)
    bias = torch.randn(128)
    e = math.floor(math.log2(fp8.FMAX[fmt] / 37.0))
    q, s = fp8.quantize(x, fmt)
    assert q.dtype == fp8.DTYPE[fmt] and float(s) == 2.0 ** -e
    assert torch.equal(q.view(torch.uint8), (x * 2.0 ** e).to(fp8.DTYPE[fmt]).view(torch.uint8))
    w8, w8t, sw = fp8.quantize_weight(w)
    assert torch.equal(w8t.view(torch.uint8), w8.view(torch.uint8).t())
    y = fp8.gemm_nt(q, s, w8, sw, bias)
    ref = ((q.float() @ w8.float().t()) * (s * sw) + bias).to(torch.bfloat16)
    assert y.dtype == torch.bfloat16 and torch.equal(y, ref)


@pytest.mark.parametrize("entry", ["single", "dist_trainer"])
def test_fp8_linear_flag_needs_amp_bf16(entry, capsys):
    import importlib
    parser = importlib.import_module("gaussiank_sgd_amd.train." + entry).build_parser()
    with pytest.raises(SystemExit):
        parser.parse_args(["--fp8-linear"])
    assert "--fp8-linear needs --amp bf16" in capsys.readouterr().err
    assert parser.parse_args(["--fp8-linear", "--amp", "bf16"]).fp8_linear
