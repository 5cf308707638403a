"""Physical boundary conditions on the device (csrc/src/kernels/boundary_fill.hip): the fast kernel of the aligned
vector layout over chunk remainders, the wave boundary, several blocks of rows, a mirror that reads the whole interior,
shared halo lines and asymmetric radii; the one-thread-per-cell kernel on the unpadded and halo-aligned layouts;
several quantities of two element sizes in one launch; sub-domains with 0, 1 and 2 physical faces; StarStencil3D with
conditions; stream order. All bitwise against the torch oracles. test_boundary.py runs the same cases
(boundary_cases.py) on the host backend."""
import pytest
import torch

import boundary_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("size", cases.SHAPE_SIZES, ids=lambda s: "RRR" if s is None else "x".join(map(str, s)))
def test_shapes(st, dev, size, radius, dtype):
    """every shape has the padded (aligned) layout, so the fast kernel is the one launched"""
    cases.case_shape(st, dev, size, radius, dtype, rot=(radius + cases.SHAPE_SIZES.index(size)) % 3)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_rotations(st, dev, rot, dtype):
    cases.case_shape(st, dev, (22, 7, 6), 3, dtype, rot)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("curr", [True, False], ids=["curr", "next"])
@pytest.mark.parametrize("with_open", [False, True], ids=["filled", "open"])
@pytest.mark.parametrize("shared", [False, True], ids=["padded", "shared"])
def test_nothing_else_is_written(st, dev, dtype, curr, with_open, shared):
    """row padding, guard and shared-line tails included (fill_bytes / buffer_to_host see every byte)"""
    cases.case_untouched(st, dev, dtype, curr, with_open, shared=shared)


@pytest.mark.parametrize("case", cases.MULTI_CASES, ids=cases.multi_id)
def test_sub_domains_and_partial_periodicity(st, dev, case):
    cases.case_multi(st, dev, *case)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("radius", cases.RADII)
@pytest.mark.parametrize("layout", ["unpadded", "x_halo_align", "shared"])
def test_layouts(st, dev, layout, radius, dtype):
    """unpadded and halo-aligned x: the generic kernel; shared halo lines: the fast kernel"""
    cases.case_layout(st, dev, layout, radius, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("shared", [False, True], ids=["padded", "shared"])
def test_asymmetric_radius(st, dev, dtype, shared):
    cases.case_asymmetric(st, dev, dtype, shared=shared)


def test_quantities(st, dev):
    cases.case_quantities(st, dev)


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (2, torch.float64), (3, torch.float32), (3, torch.float64)],
                         ids=["r1-f32", "r2-f64", "r3-f32", "r3-f64"])
@pytest.mark.parametrize("size,gpus,cost", cases.MODEL_CASES)
def test_model(st, dev, size, gpus, cost, radius, dtype):
    cases.case_model(st, dev, size, gpus, cost, radius, dtype, rot=radius % 3)


@pytest.mark.parametrize("radius,dtype", [(1, torch.float32), (3, torch.float64)], ids=["r1-f32", "r3-f64"])
def test_model_without_conditions_is_periodic(st, dev, radius, dtype):
    cases.case_model_periodic_default(st, dev, radius, dtype)


def test_fixed_point_between_two_walls(st, dev):
    cases.case_fixed_point(st, dev)


def test_mirror_conserves_the_total(st, dev):
    cases.case_conservation(st, dev)


def test_stream_order(st, dev):
    """boundary_apply on a non-default torch stream, behind a fill_ on that stream, gives the bits of the null-stream
    call: had the fill run after it, every ghost cell would hold the fill value"""
    size, R = (40, 9, 7), 2
    bc = cases.standard_bc(1)
    results = []
    for use_stream in (False, True):
        dd, (q,) = cases.make_domain(st, dev, size, st.Radius.constant(R), [torch.float32], bc)
        cases.set_field(dd, q, cases.global_field(size, torch.float32))
        t = dd.curr(0, q)
        if use_stream:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                t.fill_(0.375)
                cases.boundary_apply(dd, 0, q, stream=s.cuda_stream)
            s.synchronize()
        else:
            t.fill_(0.375)
            cases.boundary_apply(dd, 0, q)
            torch.cuda.synchronize()
        results.append(t.cpu().clone())
    assert torch.equal(results[0], results[1])
    want = cases.local_oracle(dd, 0, torch.full_like(results[0], 0.375), bc, size)
    assert torch.equal(results[1], want) and not bool((results[1] == 0.375).all())


def test_repeated_calls_reuse_the_table_and_follow_swap(st, dev):
    """the second call of a sub-domain uploads nothing new; buffer pointers travel with the launch, so after swap() the
    same table fills the other buffer"""
    size, R = (24, 6, 5), 2
    bc = cases.standard_bc(2)
    dd, (q,) = cases.make_domain(st, dev, size, st.Radius.constant(R), [torch.float64], bc)
    cases.set_field(dd, q, cases.global_field(size, torch.float64))
    dd.swap()
    cases.set_field(dd, q, cases.global_field(size, torch.float64, seed=9))
    raws = [dd.curr(0, q).cpu().clone(), dd.next(0, q).cpu().clone()]
    dd.apply_boundary()
    dd.swap()
    dd.apply_boundary()
    torch.cuda.synchronize()
    assert torch.equal(dd.next(0, q).cpu(), cases.local_oracle(dd, 0, raws[0], bc, size))
    assert torch.equal(dd.curr(0, q).cpu(), cases.local_oracle(dd, 0, raws[1], bc, size))
