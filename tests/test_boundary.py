"""Physical boundary conditions on the host backend (the plain loop of csrc/src/kernels/boundary_fill.hip), the torch
oracles of stencil2_amd.ops.reference against each other, DistributedDomain.apply_boundary and StarStencil3D with
conditions. test_gpu_boundary.py runs the same cases (boundary_cases.py) on the device."""
import pytest
import torch

import boundary_cases as cases


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("size", cases.SHAPE_SIZES, ids=lambda s: "RRR" if s is None else "x".join(map(str, s)))
def test_shapes(st, host, size, radius, dtype):
    cases.case_shape(st, host, size, radius, dtype, rot=(radius + cases.SHAPE_SIZES.index(size)) % 3)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_rotations(st, host, rot, dtype):
    cases.case_shape(st, host, (22, 7, 6), 3, dtype, rot)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("curr", [True, False], ids=["curr", "next"])
@pytest.mark.parametrize("with_open", [False, True], ids=["filled", "open"])
def test_nothing_else_is_written(st, host, dtype, curr, with_open):
    cases.case_untouched(st, host, dtype, curr, with_open)


@pytest.mark.parametrize("case", cases.MULTI_CASES, ids=cases.multi_id)
def test_sub_domains_and_partial_periodicity(st, host, case):
    cases.case_multi(st, host, *case)


def test_sub_domains_with_0_1_2_faces(st, host):
    seen = set()
    for case in cases.MULTI_CASES:
        if case[0] == (13, 11, 9) and len(case[1]) == 4 and sum(case[3]) == 2:
            seen |= cases.case_multi(st, host, *case)
    assert {0, 1, 2} <= seen, seen


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("layout", ["unpadded", "x_halo_align", "shared"])
def test_layouts(st, host, layout, radius, dtype):
    cases.case_layout(st, host, layout, radius, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_asymmetric_radius(st, host, dtype):
    cases.case_asymmetric(st, host, dtype)


def test_quantities(st, host):
    cases.case_quantities(st, host)


def test_refusals(st, host):
    cases.case_refusals(st, host)


@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (2, torch.float64), (3, torch.float32), (3, torch.float64)],
                         ids=["r1-f32", "r2-f64", "r3-f32", "r3-f64"])
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model(st, host, size, gpus, cost, radius, dtype):
    cases.case_model(st, host, size, gpus, cost, radius, dtype, rot=radius % 3)


@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (3, torch.float64)], ids=["r1-f32", "r3-f64"])
def test_model_without_conditions_is_periodic(st, host, radius, dtype):
    cases.case_model_periodic_default(st, host, radius, dtype)


def test_fixed_point_between_two_walls(st, host):
    cases.case_fixed_point(st, host)


def test_mirror_conserves_the_total(st, host):
    cases.case_conservation(st, host)


def test_default_is_periodic_and_set_boundary_alone_is_open(st, host):
    """the default state, and set_boundary alone: non-periodic faces are Open and apply_boundary writes nothing"""
    bc = st.BoundaryConditions()
    assert bc.all_periodic() and bc.boundary().all_periodic() and bc.boundary() == st.Boundary.periodic()
    assert bc.face(1, 0, 0).kind == st.FaceKind.Periodic
    dd, (q,) = cases.make_domain(st, host, (12, 6, 5), st.Radius.constant(2), [torch.float32],
                                 boundary=st.Boundary.axes(False, True, False))
    got = dd.boundary_conditions(q)
    assert got.face(-1, 0, 0).kind == st.FaceKind.Open and got.face(0, 1, 0).kind == st.FaceKind.Periodic
    assert got.boundary() == dd.boundary()
    dd.curr(0, q).fill_(cases.SENTINEL)
    assert cases.boundary_launch_info(dd, 0)["path"] == "none"
    dd.apply_boundary()
    assert bool((dd.curr(0, q) == cases.SENTINEL).all())
    # set_boundary_conditions also sets the periodic flags
    dd2, _ = cases.make_domain(st, host, (12, 6, 5), st.Radius.constant(2), [torch.float32],
                               cases.standard_bc(0, periodic=(True, False, True)))
    assert dd2.boundary() == st.Boundary.axes(True, False, True)


def test_oracles_agree_with_open_and_values(st):
    """FaceCondition constructors, and T(2.0 * v) - mirror rounds once in the field's type"""
    FC = st.FaceCondition
    assert FC.constant(1.5).value == 1.5 and FC.constant(1.5).kind == st.FaceKind.Constant
    assert FC.antimirror(0.25) == FC.antimirror(0.25) and FC.mirror() != FC.open() and FC.periodic() == FC()
    bc = st.BoundaryConditions()
    v = 0.1
    bc.set_axis(0, FC.antimirror(v), FC.antimirror(v))
    u = torch.rand((1, 1, 5), generator=torch.Generator().manual_seed(2), dtype=torch.float32)
    p = cases.pad_reference(u, 1, bc)
    c = torch.tensor(2.0 * v, dtype=torch.float64).to(torch.float32)
    assert p[0, 1, 0] == c - u[0, 0, 0] and p[0, 1, -1] == c - u[0, 0, -1]
    assert torch.equal(p[1:2, 1:2, 1:-1], u)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("boundary_apply", "boundary_launch_info", "boundary_supported", "boundary_fill_reference",
                 "pad_reference"):
        assert hasattr(ops, name), name
    for name in ("FaceKind", "FaceCondition", "BoundaryConditions"):
        assert hasattr(st, name) and hasattr(st._C, name), name
    assert hasattr(st._C, "boundary_fill") and hasattr(st._C, "boundary_fill_launch_info")
