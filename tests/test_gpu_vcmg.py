"""StarMG on the variable-coefficient operator on the device (csrc/src/kernels/stencil_varcoef_relax.hip for the
smoother and the residual, grid_transfer.hip for the coefficient of the coarser levels): one cycle bitwise against
stencil2_amd.ops.varcoef_mg_cycle_reference, convergence against the limits of vcmg_cases.py, the constructor's
refusals and two ranks sharing GPU 0. test_vcmg.py runs the same cases on the host backend."""
import os

import pytest

import vcmg_cases as cases
from conftest import run_ranks
from star_cases import dtype_id

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "vcmg_worker.py")


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=dtype_id)
def test_one_cycle_bitwise(st, dev, dtype):
    cases.case_cycle(st, dev, dtype)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence(st, dev, name):
    cases.case_convergence(st, dev, name)


def test_fp32(st, dev):
    cases.case_fp32(st, dev)


def test_jump_is_slower_but_converges(st, dev):
    cases.case_jump(st, dev)


def test_constructor_and_levels(st, dev):
    cases.case_levels(st, dev)


def test_limits(st, dev):
    cases.case_limits(st, dev)


def test_two_ranks_one_gpu():
    """two ranks sharing GPU 0: one cycle bitwise on both, and the same history bits"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "vcmg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("vcmg history ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
