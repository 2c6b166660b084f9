"""The pre-LN join (ops/ln.py ``residual_layernorm``, csrc/kernels/ln_pre.hip)
against an fp64 PyTorch reference, and gpt_tiny on it."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from gaussiank_sgd_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load(), ops._load_error


def _ln(H):
    ln = torch.nn.LayerNorm(H).cuda()
    torch.nn.init.uniform_(ln.weight, 0.5, 1.5)
    torch.nn.init.uniform_(ln.bias, -0.5, 0.5)
    return ln


def _close(got, ref, cd=F32):
    """The fp32 bound of test_add_ln_f32_vs_fp64; for a bf16 result 2**-8 |ref| more per
    element, twice the half-ulp of rounding to an 8-bit significand."""
    bound = 2e-5 * ref.abs().max() + 1e-5 + (2.0 ** -8 * ref.abs() if cd == BF16 else 0.0)
    excess = ((got.double() - ref).abs() - bound).max().item()
    print("max error over bound", excess)
    return excess <= 0


def _close_param(got, ref):
    err = (got.double() - ref).abs().max().item()
    print("parameter gradient error", err)
    return err <= 1e-5 * ref.abs().max().item() + 1e-4


# one row in a half-empty wave; chunks not a multiple of L; CH=3 / RPW=2; the first RPW=1 shape; the longest row
@pytest.mark.parametrize("with_dh", [True, False])
@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("cd", [BF16, F32])
@pytest.mark.parametrize("R,H", [(1, 8), (33, 136), (37, 768), (17, 2056), (9, 4096)])
def test_res_ln_vs_fp64(R, H, cd, with_a, with_dh, monkeypatch):
    from gaussiank_sgd_amd.ops import ln as L_
    calls = []
    orig = L_._ResLNFn.apply
    monkeypatch.setattr(L_._ResLNFn, "apply", lambda *a: calls.append(1) or orig(*a))
    torch.manual_seed(R + H)
    ln = _ln(H)
    x = torch.randn(R, H, device="cuda").requires_grad_(True)
    a = torch.randn(R, H, device="cuda").to(cd).requires_grad_(True) if with_a else None
    dy = torch.randn(R, H, device="cuda").to(cd)
    dh = torch.randn(R, H, device="cuda") if with_dh else None
    with torch.autocast("cuda", dtype=BF16, enabled=cd == BF16):
        h, y = L_.residual_layernorm(a, x, ln, 0.0, True)
    assert calls == [1] and y.dtype == cd and h.dtype == F32
    torch.autograd.backward([y, h] if with_dh else [y], [dy, dh] if with_dh else [dy])

    hr = (x.detach().double() + (a.detach().double() if with_a else 0)).requires_grad_(True)
    w = ln.weight.detach().double().requires_grad_(True)
    b = ln.bias.detach().double().requires_grad_(True)
    yr = F.layer_norm(hr, (H,), w, b, ln.eps)
    yr.backward(dy.double())
    if with_a:
        assert torch.equal(h, x.detach() + a.detach().float())
    else:
        assert h is x
    assert _close(y, yr.detach(), cd)
    dx = x.grad.double() - (dh.double() if with_dh else 0)
    assert _close(dx, hr.grad)
    if with_a:
        assert _close(a.grad, hr.grad + (dh.double() if with_dh else 0), cd)
    assert _close_param(ln.weight.grad, w.grad) and _close_param(ln.bias.grad, b.grad)


def test_res_ln_dropout_mask():
    """Kept elements are a * 1/(1-p) exactly, the backward regenerates the mask, and the mask
    is the one add_layernorm draws for the same seed."""
    from gaussiank_sgd_amd.ops.ln import _AddLNFn, _ResLNFn
    torch.manual_seed(1)
    R, H, p = 512, 768, 0.1
    ln = _ln(H)
    a = torch.randn(R, H, device="cuda").to(BF16)
    a[a == 0] = 1.0     # randn does draw an exact 0 now and then: a kept 0 would read as dropped in h
    a.requires_grad_(True)
    x = torch.zeros(R, H, device="cuda")
    h, y = _ResLNFn.apply(a, x, ln.weight, ln.bias, ln.eps, p, 1234, None, None, BF16)
    y.backward(torch.randn_like(y))
    kept = a.detach().float() * torch.tensor(1 / (1 - p), dtype=F32)
    dropped = h == 0
    assert torch.equal(h, torch.where(dropped, torch.zeros_like(kept), kept))
    assert abs(dropped.float().mean().item() - p) < 0.01
    assert torch.equal(a.grad == 0, dropped)
    a2 = a.detach().clone().requires_grad_(True)
    _AddLNFn.apply(a2, x.to(BF16), ln.weight, ln.bias, ln.eps, p, 1234, None, None, BF16).backward(torch.randn_like(y))
    assert torch.equal(a2.grad == 0, dropped)


def test_res_ln_arena_accumulation():
    from gaussiank_sgd_amd.ops.ln import _ResLNFn
    torch.manual_seed(2)
    R, H = 37, 768
    ln = _ln(H)
    a = torch.randn(R, H, device="cuda").to(BF16)
    x = torch.randn(R, H, device="cuda").requires_grad_(True)
    dy = torch.randn(R, H, device="cuda").to(BF16)
    dg, db = torch.randn(H, device="cuda"), torch.randn(H, device="cuda")
    dg0, db0 = dg.clone(), db.clone()
    for direct in ((dg, db), None):
        _ResLNFn.apply(a, x, ln.weight, ln.bias, ln.eps, 0.0, 0, direct, None, BF16)[1].backward(dy)
        if direct is not None:
            assert ln.weight.grad is None and ln.bias.grad is None
    assert _close_param(dg - dg0, ln.weight.grad.double()) and _close_param(db - db0, ln.bias.grad.double())


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gpt_tiny_on_the_fused_joins(dtype, monkeypatch):
    from gaussiank_sgd_amd.models import create_net
    from gaussiank_sgd_amd.ops import ln as L_
    torch.manual_seed(0)
    model = create_net(0, "gpt_tiny")[0].cuda().eval()
    ids = torch.randint(0, 1024, (2, 128), device="cuda")
    labels = torch.randint(0, 1024, (2, 128), device="cuda")
    calls = []
    orig = L_._ResLNFn.apply
    monkeypatch.setattr(L_._ResLNFn, "apply", lambda *a: calls.append(1) or orig(*a))

    def run():
        with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
            logits = model(ids)
            loss = F.cross_entropy(logits.float().view(-1, 1024), labels.view(-1))
        model.zero_grad(set_to_none=True)
        loss.backward()
        return logits.detach().float(), {n: p.grad.float().clone() for n, p in model.named_parameters()}

    fused, gf = run()
    assert len(calls) == 2 * len(model.blocks) + 1 == 5
    monkeypatch.setenv("GKSGD_PRELN_FUSED", "0")
    plain, gp = run()
    assert len(calls) == 5
    # the bounds of test_gpt_tiny_matches_sdpa
    tol = 5e-2 if dtype == BF16 else 1e-4
    assert (fused - plain).abs().max().item() <= tol * max(1.0, plain.abs().max().item())
    for n in gf:
        e, scale = (gf[n] - gp[n]).abs().max().item(), gp[n].abs().max().item()
        print(n, "grad diff", e, "scale", scale)
        assert e <= tol * max(1.0, scale), (n, e, scale)
