"""The StarMG V-cycle solver on the host backend: one cycle bitwise against ops.mg_cycle_reference, convergence within
the prototype's limits and along the reference's history, the level rule, the refusals, and two ranks of the TCP
group. test_gpu_mg.py runs the same cases (mg_cases.py) on the device."""
import os

import pytest

import mg_cases as cases
from algebra_cases import dtype_id
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "mg_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("box", [False, True], ids=["star", "box27"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=dtype_id)
def test_one_cycle_bitwise(st, host, dtype, box):
    cases.case_cycle(st, host, dtype, box)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence(st, host, name):
    cases.case_convergence(st, host, name)


def test_fp32_reaches_1e5(st, host):
    cases.case_fp32(st, host)


def test_level_rule(st, host):
    cases.case_levels(st, host)


def test_limits(st, host):
    cases.case_limits(st, host)


def test_two_ranks():
    """two ranks of the TCP group (host backend), several realized domains on one group: the same cycles and
    bit-identical relres on both, the solution within 1e-9 relative of the one-rank solve"""
    outs = run_ranks(2, WORKER, timeout=200)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "mg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("mg cycles ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
