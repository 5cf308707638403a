"""The fused residual / damped-Jacobi sweep of the variable-coefficient operator on the host backend (the plain loop of
csrc/src/kernels/stencil_varcoef_relax.hip) and its oracle stencil2_amd.ops.varcoef_relax_reference, bitwise.
test_gpu_relax.py runs the same cases (relax_cases.py) on the device."""
import pytest
import torch

import relax_cases as cases


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, host, size, zchunk, dtype, mode):
    cases.case_shape(st, host, size, zchunk, dtype, mode)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_residual_oracle_is_axpby_of_the_step_oracle(dtype):
    cases.case_oracle_identity(dtype)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("which", cases.DESTINATIONS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_destinations(st, host, dtype, which, mode):
    cases.case_destination(st, host, dtype, which, mode)


def test_refused_destinations(st, host):
    cases.case_refused_destinations(st, host)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, host, name, dtype):
    cases.case_sub_region(st, host, name, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_unpadded_layout(st, host, dtype):
    cases.case_generic_layout(st, host, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, host, es):
    cases.case_opaque_bytes(st, host, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_tune_flags(st, host, dtype):
    cases.case_tune_flags(st, host, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_zero_diagonal_gives_inf(st, host, dtype):
    cases.case_zero_diagonal(st, host, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_sub_domains_two_sweeps(st, host, size, gpus, cost, dtype):
    cases.case_pingpong(st, host, size, gpus, dtype, axis_cost=cost)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("walls", ["default", "constant"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_walls(st, host, dtype, walls, gpus):
    cases.case_pingpong(st, host, cases.WALL_SIZE, gpus, dtype, walls=walls)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("varcoef_relax", "varcoef_relax_supported", "varcoef_relax_launch_info", "varcoef_relax_reference",
                 "varcoef_mg_cycle_reference"):
        assert hasattr(ops, name), name
    for name in ("stencil_varcoef_relax", "stencil_varcoef_relax_supported", "stencil_varcoef_relax_launch_info"):
        assert hasattr(st._C, name), name
