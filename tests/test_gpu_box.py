"""Weighted 27-point box stencils on the device (csrc/src/kernels/stencil_box.hip): the z-march kernel of the aligned
vector layout over x / y / z remainders, wave boundaries, ring and z-chunk seams, both march directions, sub-regions,
several sub-domains per GPU (edges and corners from other sub-domains), physical walls and two ranks on one GPU, and
the one-thread-per-cell kernel on an unpadded layout; all bitwise against stencil2_amd.ops.box_step_reference.
test_box.py runs the same cases (box_cases.py) on the host backend."""
import os

import pytest
import torch

import box_cases as cases
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "box_worker.py")


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, dev, size, zchunk, dtype):
    """every shape has the padded (aligned) layout, so the z-march kernel is the one launched"""
    cases.case_shape(st, dev, size, zchunk, dtype, expect_fast=True)


def test_auto_z_chunk(st, dev):
    cases.case_auto_chunk_info(st, dev)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_march_direction(st, dev, dtype):
    cases.case_march_direction(st, dev, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("tiny", [False, True])
def test_tiny_values(st, dev, dtype, tiny):
    cases.case_tiny(st, dev, dtype, cases.TINY[dtype] if tiny else 1e-33, expect_fast=True)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_unpadded_layout_generic_kernel(st, dev, dtype):
    cases.case_generic_layout(st, dev, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, dev, es):
    cases.case_opaque_bytes(st, dev, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, dev, name, dtype):
    cases.case_sub_region(st, dev, name, dtype, expect_fast=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost,placement", cases.MODEL_CASES)
def test_model_sub_domains(st, dev, size, gpus, cost, placement, dtype, n):
    cases.case_model(st, dev, size, gpus, cost, placement, dtype, n)


@pytest.mark.parametrize("ndom", [1, 2])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_boundary_conditions(st, dev, dtype, ndom):
    """composed edge and corner ghost cells are consumed by the kernel"""
    cases.case_boundary(st, dev, dtype, ndom)


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


def test_box_from_star_matches_the_star(st, dev):
    cases.case_box_from_star(st, dev)


def test_symbol_of_the_27_point_laplacian(st, dev):
    cases.case_symbol(st, dev)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("points", cases.CG_POINTS)
@pytest.mark.parametrize("name", sorted(cases.CG_CASES))
def test_cg_on_boxes(st, dev, name, points, dtype):
    cases.case_cg(st, dev, name, points, dtype)


def test_cg_symmetry_checks(st, dev):
    cases.case_cg_symmetry(st, dev)


def test_run_until(st, dev):
    cases.case_run_until(st, dev)


def test_two_ranks_one_gpu():
    """fp32, (40, 24, 36), 4 steps on two ranks sharing GPU 0 (Colocated transport)"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("box bad 0 " in out and " of 2 " in out and "'fast'" in out for _, out in outs), outs
