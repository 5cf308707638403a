"""StarPCG on the device (field_convert.hip between the outer domain and the preconditioner's, the stencil, relax,
transfer, algebra and reduction kernels underneath): z = M r bitwise against the oracles, the solves against
ops.mgpcg_reference, options, edge cases and two ranks sharing one GPU. test_pcg.py runs the same cases (pcg_cases.py)
on the host backend."""
import os

import pytest

import pcg_cases as cases
from conftest import run_ranks
from pcg_cases import F32, F64

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "pcg_worker.py")
PRECOND = [("varcoef", F64, F32), ("varcoef", F32, F32), ("star", F64, F32), ("star", F32, F32), ("star", F64, F64)]
PRECOND_IDS = ["-".join((k, str(o).split(".")[-1], str(p).split(".")[-1])) for k, o, p in PRECOND]


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("kind,outer,precond", PRECOND, ids=PRECOND_IDS)
def test_apply_preconditioner_bitwise(st, dev, kind, outer, precond, gpus):
    cases.case_preconditioner(st, dev, kind, outer, precond, gpus)


@pytest.mark.parametrize("precond", [F64, F32], ids=["fp64_cycle", "fp32_cycle"])
@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_convergence_against_oracle(st, dev, name, precond):
    cases.case_convergence(st, dev, name, precond)


def test_convergence_two_sub_domains(st, dev):
    cases.case_convergence(st, dev, cases.POINT, F32, gpus=(0, 0))


def test_fp64_answers_from_fp32_cycles(st, dev):
    cases.case_point(st, dev)


@pytest.mark.parametrize("name", sorted(cases.CONVERGENCE))
def test_fp32_outer(st, dev, name):
    cases.case_fp32(st, dev, name)


def test_textbook_beta(st, dev):
    cases.case_not_flexible(st, dev)


@pytest.mark.parametrize("box", [False, True], ids=["star", "box"])
def test_constant_coefficients(st, dev, box):
    cases.case_constant_coefficients(st, dev, box)


def test_limits(st, dev):
    cases.case_limits(st, dev)


def test_two_ranks_one_gpu():
    """two ranks sharing GPU 0: the same (iters, relres) bits on both, the iteration count of one rank within 1"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all(" of 2 " in out and "pcg bad 0 " in out for _, out in outs), outs
    lines = [[ln for ln in out.splitlines() if ln.startswith("pcg iters ")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
