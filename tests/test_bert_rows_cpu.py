"""The cases of tests/bert_row_cases.py through the pure-PyTorch fallbacks of ops.ln.add_layernorm,
ops.xent.cross_entropy, ops.embedding.bert_embeddings and ops.linear.gelu_backward_: the cases, fp64
references and tolerance rules hold without a GPU (the HIP kernels: tests/test_bert_rows_gpu.py)."""
import pytest
import torch

import bert_row_cases as rc

CPU = torch.device("cpu")
CDS = pytest.mark.parametrize("cd", [rc.F32, rc.BF16], ids=["fp32", "bf16"])


@CDS
def test_ln_edges(cd):
    rc.scenario_ln_edges(CPU, cd)


def test_ln_buckets_written_out():
    """The bucket thresholds of the cases module: each instance covers its nc with the fewest chunks per lane."""
    for nc in range(1, 513):
        ch, rpw = rc.ln_bucket(nc)
        lanes = 64 // rpw
        assert ch * lanes >= nc, nc
        smaller = [c for c in (1, 2, 3, 4, 6, 8) if c < ch]
        assert nc > 256 or all(c * lanes < nc for c in smaller), nc
    assert {rc.ln_bucket(nc) for nc in rc.A1_NC} == {inst for _, inst in rc.LN_BUCKETS}


def test_ln_finalize():
    rc.scenario_ln_finalize(CPU)


def test_ln_offset():
    rc.scenario_ln_offset(CPU)


def test_ln_unsupported():
    rc.scenario_ln_unsupported(CPU)


@CDS
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_ln_masked_reference(cd, p):
    """A4 off the GPU: the fp64 LN(x + a * mask / (1 - p)) reference and its rules against PyTorch at the
    storage precision with a Bernoulli mask (the kernels' hash mask exists on the GPU only)."""
    t = rc.Tally("A4 ln dropout " + rc._cdname(cd))
    for H in (768, 1536, 4096):
        inp = rc.ln_inputs(37, H, cd)
        mask = torch.rand(37, H, generator=torch.Generator().manual_seed(H)) >= p
        ours = rc.ln_plain_masked(inp, mask, p)
        rbf = rc.ln_torch(inp, rc.BF16, mask, p) if cd == rc.BF16 else None
        rc.ln_check(t, "H=%d p=%g" % (H, p), ours, inp, rc.ln_torch(inp, rc.F64, mask, p),
                    rc.ln_torch(inp, rc.F32, mask, p), rbf, fused=False)
        t.true("H=%d" % H, "da must be exactly zero where dropped", not ours["da"][~mask].any())
    t.finish()


@pytest.mark.parametrize("V", rc.XENT_V)
def test_xent(V):
    rc.scenario_xent(CPU, V)


def test_xent_all_ignored_differs_from_torch():
    """The documented difference: F.cross_entropy is NaN where ours is 0.0."""
    c = rc.xent_case(6, -100, "all")
    assert torch.isnan(torch.nn.functional.cross_entropy(c.logits.float(), c.labels))
    from gaussiank_sgd_amd.ops import xent
    assert float(xent.cross_entropy(c.logits, c.labels)) == 0.0


@pytest.mark.parametrize("H", rc.EMB_H)
def test_emb_runlength(H):
    rc.scenario_emb_runlength(CPU, H)


@pytest.mark.parametrize("B", [1, 33])
def test_emb_positions(B):
    rc.scenario_emb_positions(CPU, B)


@pytest.mark.parametrize("kind", list(rc.EMB_TYPE_CASES))
def test_emb_types(kind):
    rc.scenario_emb_types(CPU, kind)


def test_emb_frozen():
    rc.scenario_emb_frozen(CPU)


def test_emb_other():
    rc.scenario_emb_other(CPU)


@CDS
def test_gelu_backward(cd):
    rc.scenario_gelu(CPU, cd)


def test_empty_inputs():
    rc.scenario_empty(CPU)
