"""The pre-LN join ``residual_layernorm`` (ops/ln.py) off the GPU: bit-equal to
the written-out composition, and gpt_tiny's restructured forward bit-equal to
what its blocks define."""
import pytest
import torch
import torch.nn.functional as F

from gaussiank_sgd_amd.ops.ln import residual_layernorm


@pytest.mark.parametrize("with_a,p,training", [(True, 0.0, True), (False, 0.0, True), (True, 0.1, True),
                                                (True, 0.1, False)])
def test_residual_layernorm_is_the_composition(with_a, p, training):
    torch.manual_seed(0)
    ln = torch.nn.LayerNorm(136)
    torch.nn.init.uniform_(ln.weight, 0.5, 1.5)
    torch.nn.init.uniform_(ln.bias, -0.5, 0.5)
    x = torch.randn(5, 7, 136)
    a = torch.randn(5, 7, 136) if with_a else None
    torch.manual_seed(11)
    h, y = residual_layernorm(a, x, ln, p, training)
    torch.manual_seed(11)
    hr = x + F.dropout(a, p, training) if with_a else x
    assert (h is x) == (not with_a)
    assert torch.equal(h, hr)
    assert torch.equal(y, ln(hr))


def test_gpt_tiny_forward_is_its_blocks():
    from gaussiank_sgd_amd.models.gpt import gpt_tiny
    torch.manual_seed(0)
    m = gpt_tiny().eval()
    ids = torch.randint(0, 1024, (2, 48))
    with torch.no_grad():
        x = m.word_embeddings(ids) + m.position_embeddings(torch.arange(48))
        for blk in m.blocks:
            x = blk(x)
        ref = F.linear(m.ln_f(x), m.word_embeddings.weight)
        assert torch.equal(m(ids), ref)
