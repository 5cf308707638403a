"""Grid transfer on the host backend (the plain loops of csrc/src/kernels/grid_transfer.hip): restriction and
prolongation bitwise against ops.restrict_reference / ops.prolong_reference over the shapes, sub-regions, operands,
layouts, walls and refusals of transfer_cases.py. test_gpu_transfer.py runs the same cases on the HIP kernels."""
import pytest
import torch

import transfer_cases as cases

DTYPES = cases.DTYPES


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size", cases.SHAPES, ids=cases.shape_id)
def test_bitwise_shapes(st, host, size, dtype):
    cases.case_shape(st, host, size, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_march_seams(st, host, dtype):
    cases.case_shape(st, host, cases.MARCH[0], dtype, zchunk=cases.MARCH[1])


@pytest.mark.parametrize("add", sorted(cases.ADDS))
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.FINE_REGIONS))
def test_prolong_regions(st, host, name, dtype, add):
    cases.case_fine_region(st, host, name, dtype, add)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.COARSE_REGIONS))
def test_restrict_regions(st, host, name, dtype):
    cases.case_coarse_region(st, host, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_unpadded_layout(st, host, dtype):
    cases.case_unpadded(st, host, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("axis", sorted(cases.CUTS))
def test_two_sub_domains(st, host, axis, dtype):
    cases.case_cut(st, host, axis, dtype)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_mixed_walls(st, host, dtype, gpus):
    cases.case_walls(st, host, dtype, gpus)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_subnormal_data(st, host, dtype):
    cases.case_tiny(st, host, dtype)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_exports(st):
    for name in ("restrict_apply", "prolong_apply", "restrict_launch_info", "prolong_launch_info",
                 "grid_transfer_supported", "restrict_reference", "prolong_reference", "mg_cycle_reference"):
        assert callable(getattr(st.ops, name)), name


def test_references_match_the_definitions():
    """R of a constant is the constant, P of a constant (periodic) is the constant, and R P is the identity on
    constants and on a linear ramp away from the wrap; P matches a direct trilinear formula"""
    from stencil2_amd.ops import prolong_reference, restrict_reference
    c = torch.full((4, 6, 8), 3.0, dtype=torch.float64)
    assert torch.equal(restrict_reference(prolong_reference(c)), c)
    g = torch.Generator().manual_seed(3)
    c = torch.rand((4, 6, 8), generator=g, dtype=torch.float64)
    p = prolong_reference(c)
    assert p.shape == (8, 12, 16)
    k, j, i = 5, 6, 9  # odd z, even y, odd x: near (2, 3, 4), far (3, 2, 5)
    def tx(K, J):
        return 0.75 * c[K, J, 4] + 0.25 * c[K, J, 5]
    def ty(K):
        return 0.75 * tx(K, 3) + 0.25 * tx(K, 2)
    assert p[k, j, i] == 0.75 * ty(2) + 0.25 * ty(3)
    add = torch.rand((8, 12, 16), generator=g, dtype=torch.float64)
    assert torch.equal(prolong_reference(c, add=add), add + p)
    f = torch.rand((8, 12, 16), generator=g, dtype=torch.float64)
    r = restrict_reference(f)
    assert r[1, 2, 3] == 0.125 * (((f[2, 4, 6] + f[2, 4, 7]) + (f[2, 5, 6] + f[2, 5, 7])) +
                                  ((f[3, 4, 6] + f[3, 4, 7]) + (f[3, 5, 6] + f[3, 5, 7])))
