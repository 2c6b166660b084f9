"""The cases of tests/bn_cases.py on the HIP kernels of bn_act.hip: through BNAct where it reaches the path,
through the raw ops (bn_stats_partials, bn_act_forward with ``pre``, bn_act_finalize, bn_act_backward_pre,
bn_relu_pool_forward / bn_relu_pool_backward) where it does not.  The same cases through the PyTorch
fallback: tests/test_bn_edges_cpu.py."""
import contextlib
import os

import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu
CDS = pytest.mark.parametrize("cd", [bc.F32, bc.BF16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def bn_blocks(cuda):
    """The module runs at the kernels' lower clamp of 64 workgroups per pass; the default is put back."""
    torch.ops.gksgd.bn_set_blocks(bc.MIN_BLOCKS)
    try:
        yield
    finally:
        torch.ops.gksgd.bn_set_blocks(int(os.environ.get("GKSGD_BN_BLOCKS", 1024)))


@contextlib.contextmanager
def at_blocks(blocks):
    torch.ops.gksgd.bn_set_blocks(blocks)
    try:
        yield blocks
    finally:
        torch.ops.gksgd.bn_set_blocks(bc.MIN_BLOCKS)


def _geo(inp, blocks):
    return bc.bn_geo(inp.M, inp.C, bc.ebytes(inp.cd), blocks)


def test_mirror_matches_workspace(cuda):
    """bn_geo against the C++ make_geo: bn_workspace_floats(M, C, eb) = 2 gy C of the 4096-workgroup grid."""
    shapes = {(s, cd) for s32, s16, _, _ in bc.G_CASES.values() for s, cd in ((s32, bc.F32), (s16, bc.BF16))}
    for cd in (bc.F32, bc.BF16):
        shapes |= {(bc.P_SHAPE[cd], cd), (bc.S_SHAPE[cd], cd), (bc.N_SHAPE, cd), (bc.P_MULTITILE[0], cd),
                   (bc.P_MORE_TILES_THAN_ROWS[0], cd), ((8, 64, 14, 14), cd), ((2, 2048, 3, 3), cd)}
    for (N, C, H, W), cd in sorted(shapes, key=str):
        if C % (8 if cd == bc.BF16 else 4) != 0:      # an fp32-only channel count
            continue
        for M in (N * H * W, bc.pool_tiles((N, C, H, W), (3, 2, 1))):
            g = bc.bn_geo(M, C, bc.ebytes(cd), bc.POOL_BLOCKS)
            assert int(torch.ops.gksgd.bn_workspace_floats(M, C, bc.ebytes(cd))) == 2 * g.gy * C, (M, C, cd, vars(g))


@CDS
@pytest.mark.parametrize("name", list(bc.G_CASES))
def test_geometry(cuda, name, cd):
    """G at 64 workgroups (where the case asks for them) and at the default; rules 1 and 2 through the raw ops."""
    inp = bc.bn_inputs(bc.g_shape(name, cd), cd)
    for blocks in bc.g_blocks(name):
        with at_blocks(blocks):
            g = _geo(inp, blocks)
            bc.scenario_geometry(cuda, name, cd, bc.depth(g))
            t = bc.Tally("G %s %s" % (name, bc.cdname(cd)))
            g2, part = bc.raw_partials(cuda, inp, blocks)
            bc.partials_check(t, "blocks=%d" % blocks, inp, g2, part)
            bc.finalize_check(t, "blocks=%d" % blocks, inp, bc.raw_finalize(cuda, inp), bc.depth(g))
            t.finish()


@CDS
def test_semantics(cuda, cd):
    inp = bc.bn_inputs(bc.S_SHAPE[cd], cd)
    bc.scenario_semantics(cuda, cd, bc.depth(_geo(inp, bc.MIN_BLOCKS)))


def test_single_value_per_channel_raises_like_torch(cuda):
    bc.scenario_single_value(cuda)


@CDS
def test_constant_channels(cuda, cd):
    """The true variance is 0: save_invstd in [1 / sqrt(|d var| + eps), 1 / sqrt(eps)] (the upper end is the clamp)."""
    D = bc.depth(_geo(bc.constant_inputs(cd), bc.MIN_BLOCKS))

    def invstd_interval(t, case, inp, dvar):
        out = bc.raw_finalize(cuda, inp)
        hi = bc.EPS ** -0.5
        lo = 1.0 / torch.sqrt(dvar + bc.EPS)
        is_ = out.invstd.double()
        print("CLAMP | %s | save_invstd / (1 / sqrt(eps)): %s" % (t.family, (is_ / hi).tolist()))
        t.true(case, "save_invstd above 1 / sqrt(eps), or NaN: var < 0 got through",
               bool((is_ <= hi * (1 + bc.FP32_SUM)).all()))
        t.true(case, "save_invstd below 1 / sqrt(|d var| + eps)", bool((is_ >= lo * (1 - bc.FP32_SUM)).all()))
        bc._elem(t, case, "save_mean", "rule2", out.mean, inp.st.mean, bc.stat_bounds(inp, D)[0])

    bc.scenario_constant(cuda, cd, D, extra=invstd_interval)


@CDS
@pytest.mark.parametrize("path", list(bc.P_POOLS))
def test_pool(cuda, path, cd):
    """P through the raw ops (argmax bytes) and BNAct(pool=...), bit-equal; statistics at the default grid."""
    with at_blocks(bc.default_blocks()) as blocks:
        bc.scenario_pool(cuda, cd, path, blocks=blocks)


def test_pool_several_tiles_per_thread(cuda):
    shape, pool = bc.P_MULTITILE
    with at_blocks(bc.default_blocks()) as blocks:
        bc.scenario_pool(cuda, bc.F32, "tile", shape=shape, pools=[pool], blocks=blocks, twins=(False,))


def test_pool_more_tiles_than_rows(cuda):
    """A 1 x 1 plane under a 4 x 4 / 2 pool with padding 2: four tiles per pixel.  The tile grid would have
    more row chunks than the workspace holds partials for, so the backward must take the per-pixel gather."""
    shape, pool = bc.P_MORE_TILES_THAN_ROWS
    with at_blocks(bc.default_blocks()) as blocks:
        bc.scenario_pool(cuda, bc.F32, "tile", shape=shape, pools=[pool], blocks=blocks)


@CDS
@pytest.mark.parametrize("mean,std", bc.N_STATS)
def test_envelope(cuda, mean, std, cd):
    """N at 64 workgroups: 6-7 (fp32) / 3-4 (bf16) rows per thread; (100, 0.1) asserts the derived bound only."""
    def raw(t, case, inp):
        g, part = bc.raw_partials(cuda, inp, bc.MIN_BLOCKS)
        bc.partials_check(t, case, inp, g, part)
        bc.finalize_check(t, case, inp, bc.raw_finalize(cuda, inp), bc.depth(g))

    bc.scenario_envelope(cuda, cd, mean, std, bc.MIN_BLOCKS, extra=raw)


@CDS
def test_forward_pre_partials(cuda, cd):
    bc.scenario_forward_pre(cuda, cd)


@CDS
@pytest.mark.parametrize("mean", [0.0, 16.0])
def test_backward_pre(cuda, cd, mean):
    bc.scenario_backward_pre(cuda, cd, mean)


def test_module_stays_at_64_workgroups(cuda):
    """at_blocks puts the module back to 64 workgroups: the partials of the multi-row shape are those of 64
    row chunks (rule 1 against that layout; raw_partials asserts that nothing is written behind them)."""
    inp = bc.bn_inputs(bc.N_SHAPE, bc.F32)
    with at_blocks(bc.default_blocks()):
        pass
    g, part = bc.raw_partials(cuda, inp, bc.MIN_BLOCKS)
    assert g.gy == 64
    t = bc.Tally("G multirow fp32")
    bc.partials_check(t, "after at_blocks", inp, g, part)
    t.finish()
