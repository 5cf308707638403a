"""The variable-coefficient diffusion stencil on the host backend (the plain loop of
csrc/src/kernels/stencil_varcoef.hip), the builders of stencil2_amd.ops.varcoef, VarCoefStencil3D and StarCG on the new
operator, bitwise against stencil2_amd.ops.varcoef_step_reference. test_gpu_varcoef.py runs the same cases
(varcoef_cases.py) on the device."""
import os

import pytest
import torch

import varcoef_cases as cases
from conftest import run_ranks

WORKER = os.path.join(os.path.dirname(__file__), "varcoef_worker.py")


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,zchunk", cases.SHAPES)
def test_shapes(st, host, size, zchunk, dtype):
    cases.case_shape(st, host, size, zchunk, dtype)


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
def test_kappa_may_be_u(st, host, dtype):
    cases.case_kappa_is_u(st, host, dtype)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model_sub_domains(st, host, size, gpus, cost, dtype, n):
    cases.case_model(st, host, size, gpus, cost, dtype, n)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("walls", ["default", "constant"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_walls(st, host, dtype, walls, gpus):
    cases.case_walls(st, host, dtype, walls, gpus)


def test_constant_coefficient_is_a_star(st, host):
    cases.case_constant_is_star(st, host)


def test_symmetry(st, host):
    cases.case_symmetry(st, host)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("walls", ["periodic", "mixed", "antimirror"])
def test_cg(st, host, walls, dtype):
    cases.case_cg(st, host, walls, dtype)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
def test_cg_inhomogeneous_wall(st, host, gpus):
    cases.case_cg(st, host, "inhomogeneous", torch.float64, gpus)


def test_run_until(st, host):
    cases.case_run_until(st, host)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_builders():
    cases.case_builders_exact()


def test_exports(st):
    import stencil2_amd.models as models
    import stencil2_amd.ops as ops
    for name in ("varcoef_apply", "varcoef_supported", "varcoef_launch_info", "varcoef_weights", "varcoef_to_lists",
                 "diffusion_varcoef", "operator_varcoef", "varcoef_step_reference"):
        assert hasattr(ops, name), name
    assert st.VarCoefStencil3D is models.VarCoefStencil3D
    for name in ("VarCoefWeights", "stencil_varcoef_apply", "stencil_varcoef_supported", "stencil_varcoef_launch_info"):
        assert hasattr(st._C, name), name


def test_two_ranks_staged():
    """fp32, (40, 24, 36), 3 steps on two ranks of the TCP group (host backend, staged transport)"""
    outs = run_ranks(2, WORKER)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("varcoef bad 0 " in out and " of 2 " in out for _, out in outs), outs
