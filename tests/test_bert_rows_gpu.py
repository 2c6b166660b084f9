"""The cases of tests/bert_row_cases.py on the HIP kernels of ln.hip, xent.hip, embed.hip and the GELU
backward of linear.hip (the same cases through the PyTorch fallbacks: tests/test_bert_rows_cpu.py)."""
import math

import pytest
import torch

import bert_row_cases as rc

pytestmark = pytest.mark.gpu
CDS = pytest.mark.parametrize("cd", [rc.F32, rc.BF16], ids=["fp32", "bf16"])
SEED = 20240611


@CDS
def test_ln_edges(cuda, cd):
    """A1; the scenario asserts that all seven (CH, RPW) instances ran, forward and backward."""
    rc.scenario_ln_edges(cuda, cd)


def test_ln_finalize(cuda):
    rc.scenario_ln_finalize(cuda)


def test_ln_offset(cuda):
    rc.scenario_ln_offset(cuda)


def test_ln_unsupported(cuda):
    rc.scenario_ln_unsupported(cuda)


@CDS
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_ln_dropout_same_mask_reference(cuda, cd, p):
    """A4: the mask recovered from the backward (a.grad == 0) and, independently, from a forward with
    a = 1, x = 0 must agree; everything against fp64 LN(x + a * mask / (1 - p)) with that mask."""
    t = rc.Tally("A4 ln dropout " + rc._cdname(cd))
    R = 37
    for H in (768, 1536, 4096):
        case = "H=%d p=%g" % (H, p)
        inp = rc.ln_inputs(R, H, cd)
        ours = rc.ln_fn(cuda, inp, p, SEED)
        dropped = (ours["da"] == 0).cpu()
        keep = rc.ln_fwd_mask(cuda, R, H, cd, p, SEED)
        t.true(case, "backward and forward masks differ in %d places" % int((dropped == keep).sum()),
               torch.equal(~dropped, keep))
        frac, sigma = float(dropped.float().mean()), math.sqrt(p * (1 - p) / (R * H))
        t.true(case, "drop fraction %.5f is not within 5 sigma (%.5f) of p" % (frac, sigma), abs(frac - p) <= 5 * sigma)
        rbf = rc.ln_torch(inp, rc.BF16, keep, p) if cd == rc.BF16 else None
        rc.ln_check(t, case, ours, inp, rc.ln_torch(inp, rc.F64, keep, p), rc.ln_torch(inp, rc.F32, keep, p), rbf)
        t.true(case, "da must be exactly zero where dropped", not ours["da"].cpu()[~keep].any())
    t.finish()


def test_ln_mask_depends_on_seed_row_column_only(cuda):
    """A5: one seed gives one mask whatever the row length (the dispatch bucket) and the storage type."""
    R, p = 37, 0.5
    masks = {(H, cd): rc.ln_fwd_mask(cuda, R, H, cd, p, SEED) for H in (768, 1536, 4096) for cd in (rc.F32, rc.BF16)}
    wide = masks[(1536, rc.F32)]
    for (H, cd), m in masks.items():
        cols = min(H, 1536)
        assert torch.equal(m[:, :cols], wide[:, :cols]), (H, cd)
        assert 0.4 < float(m.float().mean()) < 0.6
    other = rc.ln_fwd_mask(cuda, R, 1536, rc.F32, p, SEED + 1)
    assert 0.4 < float((other != wide).float().mean()) < 0.6      # an independent mask differs in about half


@CDS
@pytest.mark.parametrize("H", [264, 4096])
def test_ln_direct_arena_accumulates(cuda, cd, H):
    """A6: direct=(dg, db) views are accumulated into, and gamma / beta get no autograd gradient."""
    t = rc.Tally("A6 ln direct arena " + rc._cdname(cd))
    inp, r64, r32, rbf = rc.ln_refs(19, H, cd)
    gen = torch.Generator().manual_seed(H)
    dg0, db0 = torch.randn(H, generator=gen), torch.randn(H, generator=gen)
    dg, db = dg0.to(cuda), db0.to(cuda)
    ours = rc.ln_fn(cuda, inp, 0.0, 0, direct=(dg, db))
    assert ours["dg"] is None and ours["db"] is None
    ours["dg"], ours["db"] = dg, db
    rc.ln_check(t, "H=%d" % H, ours, inp, r64, r32, rbf, init=(dg0, db0))
    t.finish()


@pytest.mark.parametrize("V", rc.XENT_V)
def test_xent(cuda, V):
    rc.scenario_xent(cuda, V)


@pytest.mark.parametrize("H", rc.EMB_H)
def test_emb_runlength(cuda, H):
    rc.scenario_emb_runlength(cuda, H)


@pytest.mark.parametrize("B", [1, 33])
def test_emb_positions(cuda, B):
    rc.scenario_emb_positions(cuda, B)


@pytest.mark.parametrize("kind", list(rc.EMB_TYPE_CASES))
def test_emb_types(cuda, kind):
    rc.scenario_emb_types(cuda, kind)


def test_emb_frozen(cuda):
    rc.scenario_emb_frozen(cuda)


def test_emb_other(cuda):
    rc.scenario_emb_other(cuda)


@CDS
def test_gelu_backward(cuda, cd):
    rc.scenario_gelu(cuda, cd)


def test_empty_inputs(cuda):
    rc.scenario_empty(cuda)
