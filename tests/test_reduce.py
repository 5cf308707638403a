"""Field reductions on the host backend (the plain loop of csrc/src/kernels/field_reduce.hip), DistributedDomain.reduce
/ norm / dot / residual over several sub-domains and two ranks of the TCP group, and the models' run_until against the
torch oracles. test_gpu_reduce.py runs the same cases (reduce_cases.py) on the device."""
import os

import pytest
import torch

import reduce_cases as cases
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "reduce_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("a_curr,b_curr", cases.OPERANDS, ids=["curr-next", "next-curr"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_exact_shapes(st, host, case, two, a_curr, b_curr):
    cases.case_exact(st, host, case[0], case[1], two, a_curr, b_curr)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_two_buffers_of_one_quantity(st, host, dtype):
    cases.case_exact(st, host, (37, 11, 9), dtype, True, same_quantity=True)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,max_blocks", cases.FORCED)
def test_forced_grids(st, host, size, max_blocks, dtype, two):
    cases.case_forced_grid(st, host, size, dtype, two, max_blocks)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, host, name, dtype, two):
    lo, hi = cases.sub_regions((37, 11, 9))[name]
    cases.case_exact(st, host, (37, 11, 9), dtype, two, lo=lo, hi=hi)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.LAYOUTS))
def test_layouts(st, host, name, dtype, two):
    cases.case_layout(st, host, name, dtype, two)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, host, es, two):
    cases.case_opaque(st, host, es, two)


@pytest.mark.parametrize("only_nan", [False, True], ids=["nan-inf", "nan"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_nonfinite_cells(st, host, dtype, two, only_nan):
    cases.case_nonfinite(st, host, dtype, two, only_nan)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_random_within_summation_bound(st, host, dtype, two):
    cases.case_random(st, host, dtype, two)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_repeatable_bits(st, host, dtype):
    cases.case_repeatable(st, host, dtype)


def test_refusals(st, host):
    cases.case_refusals(st, host)


@pytest.mark.parametrize("gpus", [[0], [0, 0, 0]], ids=["one", "three"])
def test_sub_domains(st, host, gpus):
    cases.case_dd_exact(st, host, gpus)


def test_two_ranks_staged():
    """dd.reduce on two ranks of the TCP group (host backend): exact values on every rank, and the random field's
    struct bitwise identical on both"""
    outs = run_ranks(2, WORKER)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("reduce bad 0 " in out and " of 2 " in out for _, out in outs), outs
    hexes = [[ln for ln in out.splitlines() if ln.startswith("hex ")] for _, out in outs]
    assert len(hexes[0]) == 1 and hexes[0] == hexes[1], hexes


def test_run_until_star(st, host):
    cases.case_run_until_star(st, host)


def test_run_until_star_sub_domains(st, host):
    cases.case_run_until_star(st, host, gpus=(0, 0))


def test_run_until_jacobi(st, host):
    cases.case_run_until_jacobi(st, host)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("field_reduce", "field_reduce_launch_info", "field_reduce_supported"):
        assert hasattr(ops, name), name
    for name in ("FieldStats", "field_reduce", "field_reduce_launch_info"):
        assert hasattr(st._C, name), name
    s = st._C.FieldStats()
    assert cases.fields(s) == cases.IDENTITY and s.linf == 0.0
    for cls in (st.StarStencil3D, st.Jacobi3D, st.AstarothSim):
        assert hasattr(cls, "run_until")
    for name in ("reduce", "norm", "dot", "residual"):
        assert hasattr(st.DistributedDomain, name), name
