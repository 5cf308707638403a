"""The variable-coefficient diffusion stencil on the device (csrc/src/kernels/stencil_varcoef.hip): the z-march kernel
of the aligned vector layout over x / y / z remainders, wave boundaries, ring and z-chunk seams in both march directions
and at both buffer parities, sub-regions, several sub-domains per GPU, walls, two ranks on one GPU, StarCG on the
operator, and the one-thread-per-cell kernel on an unpadded layout; all bitwise against
stencil2_amd.ops.varcoef_step_reference. test_varcoef.py runs the same cases (varcoef_cases.py) on the host backend."""
import os

import pytest
import torch

import varcoef_cases as cases
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "varcoef_worker.py")


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
def test_kappa_may_be_u(st, dev, dtype):
    cases.case_kappa_is_u(st, dev, dtype, expect_fast=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model_sub_domains(st, dev, size, gpus, cost, dtype, n):
    cases.case_model(st, dev, size, gpus, cost, dtype, n)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("walls", ["default", "constant"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_walls(st, dev, dtype, walls, gpus):
    cases.case_walls(st, dev, dtype, walls, gpus)


def test_constant_coefficient_is_a_star(st, dev):
    cases.case_constant_is_star(st, dev)


def test_symmetry(st, dev):
    cases.case_symmetry(st, dev)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("walls", ["periodic", "mixed", "antimirror"])
def test_cg(st, dev, walls, dtype):
    cases.case_cg(st, dev, walls, dtype)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
def test_cg_inhomogeneous_wall(st, dev, gpus):
    cases.case_cg(st, dev, "inhomogeneous", torch.float64, gpus)


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


def test_two_ranks_one_gpu():
    """fp32, (40, 24, 36), 3 steps on two ranks sharing GPU 0 (Colocated transport)"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("varcoef bad 0 " in out and " of 2 " in out and "'fast'" in out for _, out in outs), outs
