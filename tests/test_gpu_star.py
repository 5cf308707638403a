"""Weighted star stencils of radius 1-3 on the device (csrc/src/kernels/stencil_star.hip): the z-march kernel of the
aligned vector layout over x / y / z remainders, wave boundaries, ring and z-chunk seams, sub-regions, several
sub-domains per GPU and two ranks on one GPU, and the one-thread-per-cell kernel on an unpadded layout; all bitwise
against stencil2_amd.ops.star_step_reference. test_star.py runs the same cases (star_cases.py) on the host backend."""
import os

import pytest
import torch

import star_cases as cases
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "star_worker.py")


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, dev, size, zchunk, radius, dtype):
    """every shape has the padded (aligned) layout, so the z-march kernel is the one launched"""
    cases.case_shape(st, dev, size, zchunk, radius, dtype, expect_fast=True)


def test_auto_z_chunk(st, dev):
    cases.case_auto_chunk_info(st, dev)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("tiny", [False, True])
def test_tiny_values(st, dev, radius, dtype, tiny):
    cases.case_tiny(st, dev, radius, dtype, cases.TINY[dtype] if tiny else 1e-33, expect_fast=True)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
def test_unpadded_layout_generic_kernel(st, dev, radius, dtype):
    cases.case_generic_layout(st, dev, radius, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, dev, es):
    cases.case_opaque_bytes(st, dev, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, dev, name, radius, dtype):
    cases.case_sub_region(st, dev, name, radius, dtype, expect_fast=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (2, torch.float64), (3, torch.float32), (3, torch.float64)],
                         ids=["r1-f32", "r2-f64", "r3-f32", "r3-f64"])
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model_sub_domains(st, dev, size, gpus, cost, radius, dtype, n):
    cases.case_model(st, dev, size, gpus, cost, radius, dtype, n)


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


def test_laplacian_error_shrinks_with_order(st, dev):
    cases.case_laplacian_order(st, dev)


def test_diffusion_is_the_astaroth_mean(st, dev):
    cases.case_diffusion_vs_astaroth(st, dev)


def test_two_ranks_one_gpu():
    """radius 3, fp32, (40, 24, 36), 4 steps on two ranks sharing GPU 0 (Colocated transport)"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("star bad 0 " in out and " of 2 " in out and "'fast'" in out for _, out in outs), outs
