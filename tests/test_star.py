"""Weighted star stencils of radius 1-3 on the host backend (the plain loop of csrc/src/kernels/stencil_star.hip), the
builders of stencil2_amd.ops.star and StarStencil3D, bitwise against stencil2_amd.ops.star_step_reference.
test_gpu_star.py runs the same cases (star_cases.py) on the device."""
import os

import pytest
import torch

import star_cases as cases
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "star_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, host, size, zchunk, radius, dtype):
    cases.case_shape(st, host, size, zchunk, radius, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("tiny", [False, True])
def test_tiny_values(st, host, radius, dtype, tiny):
    cases.case_tiny(st, host, radius, dtype, cases.TINY[dtype] if tiny else 1e-33)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
def test_unpadded_layout(st, host, radius, dtype):
    cases.case_generic_layout(st, host, radius, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, host, es):
    cases.case_opaque_bytes(st, host, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, host, name, radius, dtype):
    cases.case_sub_region(st, host, name, radius, dtype)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (2, torch.float64), (3, torch.float32), (3, torch.float64)],
                         ids=["r1-f32", "r2-f64", "r3-f32", "r3-f64"])
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model_sub_domains(st, host, size, gpus, cost, radius, dtype, n):
    cases.case_model(st, host, size, gpus, cost, radius, dtype, n)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_builders():
    cases.case_builders_exact()


def test_laplacian_error_shrinks_with_order(st, host):
    cases.case_laplacian_order(st, host)


def test_diffusion_is_the_astaroth_mean(st, host):
    cases.case_diffusion_vs_astaroth(st, host)


def test_exports(st):
    import stencil2_amd.models as models
    import stencil2_amd.ops as ops
    for name in ("star_apply", "star_supported", "star_launch_info", "star_weights", "laplacian_star", "diffusion_star",
                 "star_step_reference"):
        assert hasattr(ops, name), name
    assert st.StarStencil3D is models.StarStencil3D
    assert hasattr(st._C, "StarWeights") and hasattr(st._C, "stencil_star_apply") and hasattr(st._C, "stencil_star_supported")


def test_two_ranks_staged():
    """radius 3, fp32, (40, 24, 36), 4 steps on two ranks of the TCP group (host backend, staged transport)"""
    outs = run_ranks(2, WORKER)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("star bad 0 " in out and " of 2 " in out for _, out in outs), outs
