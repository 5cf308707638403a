"""The fused residual / damped-Jacobi sweep of the variable-coefficient operator on the device
(csrc/src/kernels/stencil_varcoef_relax.hip): the z-march kernel of the aligned vector layout over x / y / z remainders,
wave boundaries and z-chunk seams in both march directions, at both buffer parities and in both modes, every allowed
destination with the bytes around the region, sub-regions, a zero diagonal, several sub-domains per GPU, walls, and the
one-thread-per-cell kernel on an unpadded layout; all bitwise against stencil2_amd.ops.varcoef_relax_reference.
test_relax.py runs the same cases (relax_cases.py) on the host backend."""
import pytest

import relax_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, dev, size, zchunk, dtype, mode):
    """every shape has the padded (aligned) layout, so the z-march kernel is the one launched"""
    cases.case_shape(st, dev, size, zchunk, dtype, mode, expect_fast=True)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("which", cases.DESTINATIONS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_destinations(st, dev, dtype, which, mode):
    cases.case_destination(st, dev, dtype, which, mode, expect_fast=True)


def test_refused_destinations(st, dev):
    cases.case_refused_destinations(st, dev)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, dev, name, dtype):
    cases.case_sub_region(st, dev, name, dtype, expect_fast=True)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_unpadded_layout_generic_kernel(st, dev, dtype):
    cases.case_generic_layout(st, dev, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, dev, es):
    cases.case_opaque_bytes(st, dev, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_tune_flags(st, dev, dtype):
    cases.case_tune_flags(st, dev, dtype, expect_fast=True)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_zero_diagonal_gives_inf(st, dev, dtype):
    cases.case_zero_diagonal(st, dev, dtype, expect_fast=True)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_sub_domains_two_sweeps(st, dev, size, gpus, cost, dtype):
    cases.case_pingpong(st, dev, size, gpus, dtype, axis_cost=cost)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("walls", ["default", "constant"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_walls(st, dev, dtype, walls, gpus):
    cases.case_pingpong(st, dev, cases.WALL_SIZE, gpus, dtype, walls=walls)


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)
