"""The StarMG V-cycle solver on the device (grid_transfer.hip, stencil_star.hip / stencil_box.hip, field_axpby.hip):
one cycle bitwise against ops.mg_cycle_reference, convergence within the prototype's limits and along the reference's
history, the level rule, the refusals, and two ranks sharing GPU 0. test_mg.py runs the same cases (mg_cases.py) on
the host backend."""
import os

import pytest

import mg_cases as cases
from algebra_cases import dtype_id
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "mg_worker.py")


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("box", [False, True], ids=["star", "box27"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=dtype_id)
def test_one_cycle_bitwise(st, dev, dtype, box):
    cases.case_cycle(st, dev, dtype, box)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence(st, dev, name):
    m = cases.case_convergence(st, dev, name)
    from stencil2_amd.ops import prolong_launch_info, restrict_launch_info
    for di in range(m.domain.num_domains()):
        fine, coarse = m.level_domain(0), m.level_domain(1)
        assert restrict_launch_info(fine, coarse, di, m.r, m.f)["path"] == "fast"
        assert prolong_launch_info(coarse, fine, di, m.u, m.u, add=m.u)["path"] == "fast"


def test_fp32_reaches_1e5(st, dev):
    cases.case_fp32(st, dev)


def test_level_rule(st, dev):
    cases.case_levels(st, dev)


def test_limits(st, dev):
    cases.case_limits(st, dev)


def test_two_ranks_one_gpu():
    """two ranks sharing GPU 0, several realized domains on one group: the same cycles and bit-identical relres on
    both, the solution within 1e-9 relative of the one-rank solve"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "mg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("mg cycles ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
