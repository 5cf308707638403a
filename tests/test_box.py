"""Weighted 27-point box stencils on the host backend (the plain loop of csrc/src/kernels/stencil_box.hip), the builders
of stencil2_amd.ops.box, BoxStencil3D and StarCG on boxes, bitwise against stencil2_amd.ops.box_step_reference.
test_gpu_box.py runs the same cases (box_cases.py) on the device."""
import os

import pytest
import torch

import box_cases as cases
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "box_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, host, size, zchunk, dtype):
    cases.case_shape(st, host, size, zchunk, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("tiny", [False, True])
def test_tiny_values(st, host, dtype, tiny):
    cases.case_tiny(st, host, dtype, cases.TINY[dtype] if tiny else 1e-33)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_unpadded_layout(st, host, dtype):
    cases.case_generic_layout(st, host, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, host, es):
    cases.case_opaque_bytes(st, host, es)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, host, name, dtype):
    cases.case_sub_region(st, host, name, dtype)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost,placement", cases.MODEL_CASES)
def test_model_sub_domains(st, host, size, gpus, cost, placement, dtype, n):
    cases.case_model(st, host, size, gpus, cost, placement, dtype, n)


@pytest.mark.parametrize("ndom", [1, 2])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_boundary_conditions(st, host, dtype, ndom):
    """composed edge and corner ghost cells are consumed by the stencil"""
    cases.case_boundary(st, host, dtype, ndom)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_builders():
    cases.case_builders_exact()


def test_box_from_star_matches_the_star(st, host):
    cases.case_box_from_star(st, host)


def test_symbol_of_the_27_point_laplacian(st, host):
    cases.case_symbol(st, host)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("points", cases.CG_POINTS)
@pytest.mark.parametrize("name", sorted(cases.CG_CASES))
def test_cg_on_boxes(st, host, name, points, dtype):
    cases.case_cg(st, host, name, points, dtype)


def test_cg_symmetry_checks(st, host):
    cases.case_cg_symmetry(st, host)


def test_run_until(st, host):
    cases.case_run_until(st, host)


def test_exports(st):
    import stencil2_amd.models as models
    import stencil2_amd.ops as ops
    for name in ("box_apply", "box_supported", "box_launch_info", "box_weights", "box_to_lists", "box_from_star",
                 "laplacian_box", "diffusion_box", "smoothing_box", "box_step_reference"):
        assert hasattr(ops, name), name
    assert st.BoxStencil3D is models.BoxStencil3D
    assert hasattr(st._C, "BoxWeights") and hasattr(st._C, "stencil_box_apply") and hasattr(st._C, "stencil_box_supported")


def test_two_ranks_staged():
    """fp32, (40, 24, 36), 4 steps on two ranks of the TCP group (host backend, staged transport)"""
    outs = run_ranks(2, WORKER)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("box bad 0 " in out and " of 2 " in out for _, out in outs), outs
