"""The cases of tests/lstm_cases.py on the HIP kernels of lstm.hip, through the raw ops ``lstm_rec_gemm``,
``lstm_rec_gemm_x6``, ``lstm_cell_fwd`` and ``lstm_cell_bwd``.  The same cases through the torch mirrors and
the PyTorch fallback: tests/test_lstm_edges_cpu.py.  Measured ratios: profiles/lstm_kernels_tolerances.txt."""
import pytest

import lstm_cases as lc

pytestmark = pytest.mark.gpu
CDS = pytest.mark.parametrize("cd", [lc.F32, lc.BF16], ids=["fp32", "bf16"])
KINDS = pytest.mark.parametrize("kind", lc.KINDS)


@KINDS
def test_gemm_exact(cuda, kind):
    lc.scenario_gemm_exact(cuda, kind)


@KINDS
def test_gemm_random(cuda, kind):
    lc.scenario_gemm_random(cuda, kind)


@KINDS
def test_gemm_strided(cuda, kind):
    lc.scenario_gemm_strided(cuda, kind)


@KINDS
def test_gemm_refusals(cuda, kind):
    lc.scenario_gemm_refusals(cuda, kind)


@CDS
def test_cell_forward(cuda, cd):
    lc.scenario_cell_fwd(cuda, cd)


@CDS
def test_cell_backward(cuda, cd):
    lc.scenario_cell_bwd(cuda, cd)


@CDS
def test_cell_saturation(cuda, cd):
    lc.scenario_cell_saturation(cuda, cd)


@CDS
def test_cell_refusals(cuda, cd):
    lc.scenario_cell_refusals(cuda, cd)
