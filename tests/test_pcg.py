"""StarPCG on the host backend: z = M r bitwise against the oracles, the solves against ops.mgpcg_reference, options,
edge cases and two ranks of the TCP group. test_gpu_pcg.py runs the same cases (pcg_cases.py) on the device."""
import os

import pytest

import pcg_cases as cases
from conftest import run_ranks
from pcg_cases import F32, F64

WORKER = os.path.join(os.path.dirname(__file__), "pcg_worker.py")
PRECOND = [("varcoef", F64, F32), ("varcoef", F32, F32), ("star", F64, F32), ("star", F32, F32), ("star", F64, F64)]
PRECOND_IDS = ["-".join((k, str(o).split(".")[-1], str(p).split(".")[-1])) for k, o, p in PRECOND]


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_oracle_stays_inside_the_caps(name):
    cases.case_oracle_caps(name)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("kind,outer,precond", PRECOND, ids=PRECOND_IDS)
def test_apply_preconditioner_bitwise(st, host, kind, outer, precond, gpus):
    cases.case_preconditioner(st, host, kind, outer, precond, gpus)


@pytest.mark.parametrize("precond", [F64, F32], ids=["fp64_cycle", "fp32_cycle"])
@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence_against_oracle(st, host, name, precond):
    cases.case_convergence(st, host, name, precond)


def test_convergence_two_sub_domains(st, host):
    cases.case_convergence(st, host, cases.POINT, F32, gpus=(0, 0))


def test_fp64_answers_from_fp32_cycles(st, host):
    cases.case_point(st, host)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_fp32_outer(st, host, name):
    cases.case_fp32(st, host, name)


def test_textbook_beta(st, host):
    cases.case_not_flexible(st, host)


@pytest.mark.parametrize("box", [False, True], ids=["star", "box"])
def test_constant_coefficients(st, host, box):
    cases.case_constant_coefficients(st, host, box)


def test_limits(st, host):
    cases.case_limits(st, host)


def test_two_ranks_staged():
    """two ranks of the TCP group (host backend): the same (iters, relres) bits on both ranks, and the iteration count
    of one rank within 1"""
    outs = run_ranks(2, WORKER)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "pcg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("pcg iters ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines


def test_exports(st):
    import stencil2_amd.ops as ops
    assert hasattr(ops, "mgpcg_reference") and hasattr(st, "StarPCG") and "StarPCG" in st.__all__
