"""StarMG on the variable-coefficient operator, host backend: one cycle bitwise against
stencil2_amd.ops.varcoef_mg_cycle_reference, the coefficient of every level, convergence against the limits of
vcmg_cases.py, the constructor's refusals and two ranks of the TCP group. test_gpu_vcmg.py runs the same cases on the
device."""
import os

import pytest

import vcmg_cases as cases
from conftest import run_ranks
from star_cases import dtype_id

WORKER = os.path.join(os.path.dirname(__file__), "vcmg_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=dtype_id)
def test_one_cycle_bitwise(st, host, dtype):
    cases.case_cycle(st, host, dtype)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence(st, host, name):
    cases.case_convergence(st, host, name)


def test_fp32(st, host):
    cases.case_fp32(st, host)


def test_jump_is_slower_but_converges(st, host):
    cases.case_jump(st, host)


def test_constructor_and_levels(st, host):
    cases.case_levels(st, host)


def test_limits(st, host):
    cases.case_limits(st, host)


def test_two_ranks():
    """two ranks of the TCP group (host backend): one cycle bitwise on both, and the same history bits"""
    outs = run_ranks(2, WORKER, timeout=200)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "vcmg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("vcmg history ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
