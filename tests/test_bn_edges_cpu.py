"""The cases of tests/bn_cases.py through BNAct's PyTorch fallback: the fp64 references, the geometry mirror's
case table and the tolerance rules hold without a GPU (the HIP kernels: tests/test_bn_edges_gpu.py).  The
depths D of the rules are those of the kernel's geometry at the default number of workgroups."""
import pytest
import torch

import bn_cases as bc

CPU = torch.device("cpu")
CDS = pytest.mark.parametrize("cd", [bc.F32, bc.BF16], ids=["fp32", "bf16"])


def _depth(shape, cd, blocks=None):
    N, C, H, W = shape
    return bc.depth(bc.bn_geo(N * H * W, C, bc.ebytes(cd), blocks or bc.default_blocks()))


def test_case_table_reaches_every_property():
    bc.assert_case_table()


def test_geometry_mirror_by_hand():
    """The figures of three launches worked out by hand from make_geo."""
    g = bc.bn_geo(8 * 14 * 14, 64, 4, 1024)
    assert (g.tpr, g.rl, g.gx, g.gy, g.rpb) == (16, 16, 1, 98, 16)
    g = bc.bn_geo(2 * 3 * 3, 2048, 4, 1024)
    assert (g.tpr, g.rl, g.gx, g.gy, g.rpb) == (64, 4, 8, 5, 4)
    g = bc.bn_geo(3 * 17 * 13, 268, 4, 1024)
    assert (g.tpr, g.rl, g.gx) == (1, 256, 67) and bc.idle_lanes(g) == 0
    assert bc.idle_lanes(bc.bn_geo(105, 40, 4, 1024)) == 6


@CDS
@pytest.mark.parametrize("name", list(bc.G_CASES))
def test_geometry(name, cd):
    bc.scenario_geometry(CPU, name, cd, _depth(bc.g_shape(name, cd), cd))


@CDS
def test_semantics(cd):
    bc.scenario_semantics(CPU, cd, _depth(bc.S_SHAPE[cd], cd))


def test_single_value_per_channel_raises_like_torch():
    bc.scenario_single_value(CPU)


@CDS
def test_constant_channels(cd):
    """PyTorch's CPU reduction of a channels-last tensor of 4 or 8 channels is one fp32 chain over the rows
    (its mean of 17956 copies of 300.3 is off by 7e-3): the depth of rule 2 is M here, not the kernel's."""
    bc.scenario_constant(CPU, cd, bc.constant_inputs(cd).M)


@CDS
@pytest.mark.parametrize("path", list(bc.P_POOLS))
def test_pool(path, cd):
    """Rule 5's cap on undecided windows holds for the chosen seeds with the PyTorch composition as ours."""
    bc.scenario_pool(CPU, cd, path)


def test_pool_more_tiles_than_rows():
    shape, pool = bc.P_MORE_TILES_THAN_ROWS
    bc.scenario_pool(CPU, bc.F32, "tile", shape=shape, pools=[pool])


@CDS
@pytest.mark.parametrize("mean,std", bc.N_STATS)
def test_envelope(mean, std, cd):
    bc.scenario_envelope(CPU, cd, mean, std, bc.MIN_BLOCKS)
