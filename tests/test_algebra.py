"""Field algebra on the host backend (the plain loop of csrc/src/kernels/field_axpby.hip), DistributedDomain.axpby /
copy / scale over several sub-domains and two ranks of the TCP group, and the StarCG solver against a torch CG.
test_gpu_algebra.py runs the same cases (algebra_cases.py) on the device."""
import os

import pytest
import torch

import algebra_cases as cases
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "algebra_worker.py")
DTYPES = [torch.float32, torch.float64]


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_bitwise_shapes(st, host, case):
    cases.case_shape(st, host, case[0], case[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size", cases.ALIAS_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(cases.ALIASES))
def test_aliasing(st, host, name, size, dtype):
    cases.case_alias(st, host, size, dtype, name)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.regions((37, 11, 9))))
def test_untouched_bytes(st, host, name, dtype, stats):
    cases.case_region(st, host, name, dtype, stats)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.rc.LAYOUTS))
def test_layouts(st, host, name, dtype):
    cases.case_layout(st, host, name, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, host, es):
    cases.case_opaque(st, host, es)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,max_blocks", cases.FORCED)
def test_forced_grids(st, host, size, max_blocks, dtype):
    cases.case_forced_grid(st, host, size, dtype, max_blocks)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_stats_exact(st, host, case, two):
    cases.case_stats_exact(st, host, case[0], case[1], two)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_random_within_summation_bound(st, host, dtype):
    cases.case_stats_random(st, host, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_nonfinite(st, host, dtype):
    cases.case_stats_nonfinite(st, host, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_repeatable_bits(st, host, dtype):
    cases.case_stats_repeatable(st, host, dtype)


def test_refusals(st, host):
    cases.case_refusals(st, host)


@pytest.mark.parametrize("gpus", [[0], [0, 0, 0]], ids=["one", "three"])
def test_sub_domains(st, host, gpus):
    cases.case_dd(st, host, gpus)


def test_two_ranks_staged():
    """dd.axpby with stats and StarCG on two ranks of the TCP group (host backend): exact values on every rank, the
    random field's struct and the solver's (iters, relres) bitwise identical on both"""
    outs = run_ranks(2, WORKER)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("axpby bad 0 " in out and " of 2 " in out for _, out in outs), outs
    for prefix in ("hex ", "cg iters "):
        lines = [[ln for ln in out.splitlines() if ln.startswith(prefix)] for _, out in outs]
        assert len(lines[0]) == 1 and lines[0] == lines[1], lines


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.CG_CASES))
def test_cg(st, host, name, dtype):
    cases.case_cg(st, host, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_cg_sub_domains(st, host, dtype):
    cases.case_cg(st, host, "helmholtz_walls", dtype, gpus=(0, 0))


def test_cg_limits(st, host):
    cases.case_cg_limits(st, host)


def test_wall_second_order(st, host):
    cases.case_wall_order(st, host)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("field_axpby", "field_axpby_launch_info", "field_axpby_supported", "axpby_reference"):
        assert hasattr(ops, name), name
    for name in ("field_axpby", "field_axpby_launch_info", "field_axpby_supported"):
        assert hasattr(st._C, name), name
    for name in ("axpby", "copy", "scale"):
        assert hasattr(st.DistributedDomain, name), name
    assert hasattr(st, "StarCG") and "StarCG" in st.__all__
