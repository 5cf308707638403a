"""Cases shared by test_boundary.py (host backend, the plain loop) and test_gpu_boundary.py (the HIP kernel of
csrc/src/kernels/boundary_fill.hip): ghost-cell fill for the non-periodic faces of the global grid. Every comparison
is bitwise unless a case says otherwise, against the torch oracles of stencil2_amd.ops.reference:
boundary_fill_reference (the composed z, y, x map on one sub-domain's raw tensor) and pad_reference (sequential
padding of the global grid).

Fields are seeded torch.rand; condition values are distinct seeded numbers in (-2, 2). The standard assignment of kinds
(-x Mirror, +x AntiMirror, -y Constant, +y Mirror, -z AntiMirror, +z Constant) and its two rotations bring every kind
onto every axis."""
import functools
import math

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (boundary_apply, boundary_fill_reference, boundary_launch_info, boundary_supported,
                              diffusion_star, pad_reference, star_step_reference)

from star_cases import global_field, oracle as periodic_star_oracle, random_weights

FC = _C.FaceCondition
SENTINEL = -777.25
RADII = [1, 2, 3]
DTYPES = [torch.float32, torch.float64]
SHAPE_SIZES = [(20, 6, 5), (21, 6, 5), (22, 6, 5), (23, 6, 5),  # chunk remainders
               (255, 6, 5), (256, 6, 5), (257, 6, 5),          # the wave boundary
               (24, 17, 5), (24, 6, 9),                        # more than one block of rows in y / z
               None]                                           # (R, R, R): the mirror reads the whole interior


def dtype_id(dt):
    return str(dt).split(".")[-1]


def values(seed):
    """four distinct condition values in (-2, 2)"""
    v = (torch.rand(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 4 - 2).tolist()
    assert len(set(v)) == 4
    return v


def standard_bc(rot=0, periodic=(False, False, False), seed=41):
    """the standard assignment rotated by `rot` axes; axes in `periodic` stay periodic"""
    v1, v2, v3, v4 = values(seed)
    pairs = [(FC.mirror(), FC.antimirror(v1)), (FC.constant(v2), FC.mirror()), (FC.antimirror(v3), FC.constant(v4))]
    bc = _C.BoundaryConditions()
    for ax in range(3):
        if not periodic[ax]:
            lo, hi = pairs[(ax + rot) % 3]
            bc.set_axis(ax, lo, hi)
    return bc


def all_faces(cond_lo, cond_hi=None):
    bc = _C.BoundaryConditions()
    for ax in range(3):
        bc.set_axis(ax, cond_lo, cond_hi if cond_hi is not None else cond_lo)
    return bc


def _sync(dd):
    if dd.backend() == _C.Backend.Device:
        torch.cuda.synchronize()


def make_domain(st, backend, size, radius, dtypes, bc=None, gpus=(0,), axis_cost=None, padding=True, x_halo_align=False,
                shared=False, overrides=None, boundary=None):
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius)
    dd.set_gpus(list(gpus))
    if axis_cost is not None:
        dd.set_axis_cost(st.Dim3(*axis_cost))
    if not padding:
        dd.set_padding(False)
    if x_halo_align:
        dd.set_x_halo_align(True)
    if shared:
        dd.set_shared_halo_line(True)
    qs = [dd.add_data(f"u{i}", dt) for i, dt in enumerate(dtypes)]
    if boundary is not None:
        dd.set_boundary(boundary)
    if bc is not None:
        dd.set_boundary_conditions(bc)
    for q, b in (overrides or {}).items():
        dd.set_boundary_conditions(q, b)
    dd.realize()
    assert dd.num_domains() == len(gpus)
    return dd, qs


def set_field(dd, q, u):
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        t = dd.curr_interior(di, q)
        t.copy_(u[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x].to(t.device))
    _sync(dd)


def geometry(dd, di):
    d = dd.domain(di)
    o, s, r = d.origin(), d.size(), d.radius()
    return ((o.x, o.y, o.z), (s.x, s.y, s.z), (r.x(-1), r.y(-1), r.z(-1)), (r.x(1), r.y(1), r.z(1)))


def local_oracle(dd, di, raw, bc, grid, return_mask=False):
    origin, size, rlo, rhi = geometry(dd, di)
    return boundary_fill_reference(raw, origin, size, rlo, rhi, grid, bc, return_mask=return_mask)


def pad_window(dd, di, padded, R):
    """the part of the padded global grid (pad R on every side) that sub-domain di's raw tensor covers"""
    origin, size, rlo, rhi = geometry(dd, di)
    assert rlo == (R,) * 3 and rhi == (R,) * 3
    return padded[origin[2]:origin[2] + size[2] + 2 * R, origin[1]:origin[1] + size[1] + 2 * R,
                  origin[0]:origin[0] + size[0] + 2 * R]


def expect_path(backend, info, device_path):
    want = device_path if backend == _C.Backend.Device else "host"
    assert info["path"] == want, info


# ---- 1. shapes: one sub-domain, all faces non-periodic ----
def case_shape(st, backend, size, R, dtype, rot):
    size = size if size is not None else (R, R, R)
    bc = standard_bc(rot)
    dd, (q,) = make_domain(st, backend, size, st.Radius.constant(R), [dtype], bc)
    u = global_field(size, dtype)
    set_field(dd, q, u)
    dd.exchange()
    _sync(dd)
    raw = dd.curr(0, q).cpu().clone()
    info = boundary_launch_info(dd, 0)
    expect_path(backend, info, "fast")
    # six slabs; the fast kernel takes both x sides of a row in one item, so its two x slabs are one box
    assert info["boxes"] == (5 if backend == _C.Backend.Device else 6), info
    if backend == _C.Backend.Device:
        assert info["launches"] == 1 and info["blocks"] >= 5, info
    dd.apply_boundary()
    _sync(dd)
    got = dd.curr(0, q).cpu()
    want = local_oracle(dd, 0, raw, bc, size)
    bad = int((got != want).sum())
    assert bad == 0 and torch.equal(got, want), f"{bad} cells differ from the composed map ({info})"
    assert torch.equal(got, pad_reference(u, R, bc)), "differs from sequential padding of the global grid"


# ---- 2. nothing else is written ----
def byte_mask(d, q, mask):
    """bytes of buffer_to_host(q) that belong to the cells of the raw (z, y, x) boolean `mask`"""
    es, p, pad = d.elem_size(q), d.pitch(q), d.pad_x(q)
    z, y, x = np.nonzero(mask.numpy())
    first = (pad + x + p.x * (y + p.y * z)) * es
    n = len(d.buffer_to_host(q, True))
    out = np.zeros(n, dtype=bool)
    for b in range(es):
        out[first + b] = True
    return out


def case_untouched(st, backend, dtype, curr, with_open, shared=False):
    size, R = (22, 7, 6), 2
    if with_open:
        bc = standard_bc(1)
        bc.set_axis(0, FC.open(), FC.open())
        bc.set_face(0, 0, 1, FC.open())
    else:
        bc = standard_bc(0)
    dd, (q,) = make_domain(st, backend, size, st.Radius.constant(R), [dtype], bc, shared=shared)
    d = dd.domain(0)
    d.fill_bytes(q, 0xAB, True, True)
    u = global_field(size, dtype)
    if not curr:
        dd.swap()
    set_field(dd, q, u)  # the buffer that is filled holds the field
    if not curr:
        dd.swap()
    _sync(dd)
    before = [np.frombuffer(d.buffer_to_host(q, c), dtype=np.uint8).copy() for c in (True, False)]
    raw = (dd.curr(0, q) if curr else dd.next(0, q)).cpu().clone()
    dd.apply_boundary(q, curr)
    _sync(dd)
    after = [np.frombuffer(d.buffer_to_host(q, c), dtype=np.uint8).copy() for c in (True, False)]
    want, mask = local_oracle(dd, 0, raw, bc, size, return_mask=True)
    got = (dd.curr(0, q) if curr else dd.next(0, q)).cpu()
    assert torch.equal(got, want)
    assert int(mask.sum()) > 0
    filled, other = (0, 1) if curr else (1, 0)
    assert np.array_equal(after[other], before[other]), "the other buffer was written"
    ghost_bytes = byte_mask(d, q, mask)
    changed = after[filled] != before[filled]
    assert not (changed & ~ghost_bytes).any(), f"{int((changed & ~ghost_bytes).sum())} bytes outside the ghost cells changed"
    if with_open:
        # the cells beyond the open +z face (z resolves first), and the cells beyond the open x faces that lie beyond
        # no other face, are as they were; the y pass of the definition does cover the whole raw x
        assert torch.equal(got[-R:], raw[-R:]) and not mask[-R:].any()
        inner = (slice(R, -R), slice(R, -R))
        assert torch.equal(got[inner][:, :, :R], raw[inner][:, :, :R]) and torch.equal(got[inner][:, :, -R:], raw[inner][:, :, -R:])
        assert not mask[inner][:, :, :R].any() and not mask[inner][:, :, -R:].any()
        assert mask[R:-R, :R].all() and mask[:R].all()


# ---- 3. several sub-domains and partial periodicity ----
MULTI_CASES = [(size, gpus, cost, per)
               for size in ((13, 11, 9), (45, 10, 8))
               for gpus in ([0, 0], [0, 0, 0, 0])
               for cost in ((1, 100, 100), (100, 1, 100), (100, 100, 1))  # the cheapest axis takes every cut
               for per in ((False, True, True), (True, False, True), (True, True, False), (False, False, False))]


def multi_id(c):
    size, gpus, cost, per = c
    return f"{'x'.join(map(str, size))}-{len(gpus)}-cut{min(range(3), key=lambda a: cost[a])}-{''.join('T' if p else 'F' for p in per)}"


def case_multi(st, backend, size, gpus, cost, per, dtype=torch.float32):
    R = 2
    bc = standard_bc(sum(size) % 3, periodic=per)
    dd, (q,) = make_domain(st, backend, size, st.Radius.constant(R), [dtype], bc, gpus=gpus, axis_cost=cost)
    cut = min(range(3), key=lambda a: cost[a])
    dim = dd.placement_dim()
    assert (dim.x, dim.y, dim.z)[cut] == len(gpus)
    u = global_field(size, dtype)
    set_field(dd, q, u)
    dd.exchange()
    _sync(dd)
    raws = [dd.curr(di, q).cpu().clone() for di in range(dd.num_domains())]
    faces_seen = set()
    for di in range(dd.num_domains()):
        origin, sz, _, _ = geometry(dd, di)
        faces = sum((not per[a]) * ((origin[a] == 0) + (origin[a] + sz[a] == size[a])) for a in range(3))
        faces_seen.add(faces)
        info = boundary_launch_info(dd, di)
        if faces == 0:
            assert info["path"] == "none" and info["launches"] == 0 and info["boxes"] == 0, info
        else:
            expect_path(backend, info, "fast")
            both_x = not per[0] and origin[0] == 0 and origin[0] + sz[0] == size[0]
            assert info["boxes"] == faces - (1 if both_x and backend == _C.Backend.Device else 0), info
            if backend == _C.Backend.Device:
                assert info["launches"] == 1, info
    dd.apply_boundary()
    _sync(dd)
    padded = pad_reference(u, R, bc)
    for di in range(dd.num_domains()):
        got = dd.curr(di, q).cpu()
        assert torch.equal(got, local_oracle(dd, di, raws[di], bc, size)), f"sub-domain {di}: the composed map"
        # radius R in all 26 directions: every source cell is exchanged, so the whole raw tensor is the global padding
        assert torch.equal(got, pad_window(dd, di, padded, R)), f"sub-domain {di}: sequential padding"
    return faces_seen


# ---- 4. layouts ----
def case_layout(st, backend, layout, R, dtype):
    size = (21, 9, 7)
    kw = {"unpadded": dict(padding=False), "x_halo_align": dict(x_halo_align=True), "shared": dict(shared=True)}[layout]
    bc = standard_bc(R % 3)
    dd, (q,) = make_domain(st, backend, size, st.Radius.constant(R), [dtype], bc, **kw)
    if layout == "shared":
        assert dd.domain(0).shared_halo_line()
    u = global_field(size, dtype)
    set_field(dd, q, u)
    dd.exchange()
    _sync(dd)
    raw = dd.curr(0, q).cpu().clone()
    expect_path(backend, boundary_launch_info(dd, 0), "fast" if layout == "shared" else "generic")
    dd.apply_boundary()
    _sync(dd)
    got = dd.curr(0, q).cpu()
    assert torch.equal(got, local_oracle(dd, 0, raw, bc, size))
    assert torch.equal(got, pad_reference(u, R, bc))


def case_asymmetric(st, backend, dtype, shared=False):
    """face radii -x 1, +x 3, the others 2; edges and corners 1"""
    size = (22, 7, 6)
    r = st.Radius.face_edge_corner(2, 1, 1)
    r.set_dir(-1, 0, 0, 1)
    r.set_dir(1, 0, 0, 3)
    for rot in range(3):
        bc = standard_bc(rot)
        dd, (q,) = make_domain(st, backend, size, r, [dtype], bc, shared=shared)
        set_field(dd, q, global_field(size, dtype))
        dd.exchange()
        _sync(dd)
        raw = dd.curr(0, q).cpu().clone()
        assert tuple(raw.shape) == (size[2] + 4, size[1] + 4, size[0] + 4)
        expect_path(backend, boundary_launch_info(dd, 0), "fast")
        dd.apply_boundary()
        _sync(dd)
        want, mask = local_oracle(dd, 0, raw, bc, size, return_mask=True)
        assert torch.equal(dd.curr(0, q).cpu(), want)
        assert mask[:, :, :1].all() and mask[:, :, -3:].all() and not mask[2:-2, 2:-2, 1:-3].any()


# ---- 5. quantities ----
def case_quantities(st, backend):
    size, R = (23, 6, 5), 2
    bc = standard_bc(0)
    bc1 = standard_bc(2, seed=77)  # the override of quantity 1: other kinds per face, other values
    open_bc = all_faces(FC.open())
    dtypes = [torch.float32, torch.float32, torch.float64, torch.int32]
    dd, qs = make_domain(st, backend, size, st.Radius.constant(R), dtypes, bc, overrides={1: bc1, 3: open_bc})
    bcs = [bc, bc1, bc, open_bc]
    for q in qs:
        assert dd.boundary_conditions(q) == bcs[q]
    for q in qs[:3]:
        set_field(dd, q, global_field(size, dtypes[q], seed=5 + q))
    dd.curr(0, 3).fill_(-12345)
    dd.exchange()
    _sync(dd)
    raws = [dd.curr(0, q).cpu().clone() for q in qs]
    info = boundary_launch_info(dd, 0)
    expect_path(backend, info, "fast")
    # three quantities with six faces each (the fast kernel: five boxes each); the Open one has no item
    assert info["boxes"] == (15 if backend == _C.Backend.Device else 18), info
    if backend == _C.Backend.Device:
        assert info["launches"] == 1, info  # fp32 and fp64 items share the launch
    assert boundary_launch_info(dd, 0, q=3)["path"] == "none"
    assert boundary_supported(dd, 0, 3) and not boundary_supported(dd, 0, 3, bc)
    dd.apply_boundary()
    _sync(dd)
    for q in qs[:3]:
        got = dd.curr(0, q).cpu()
        assert torch.equal(got, local_oracle(dd, 0, raws[q], bcs[q], size)), f"quantity {q}"
        assert not torch.equal(got, raws[q])
    assert torch.equal(dd.curr(0, 3).cpu(), raws[3]) and bool((dd.curr(0, 3) == -12345).all())
    # the same through ops.boundary_apply with explicit lists, into fresh ghost cells
    for q in qs[:3]:
        dd.curr(0, q).copy_(raws[q].to(dd.curr(0, q).device))
    _sync(dd)
    boundary_apply(dd, 0, [0, 1, 2], [bc, bc1, bc])
    _sync(dd)
    for q in qs[:3]:
        assert torch.equal(dd.curr(0, q).cpu(), local_oracle(dd, 0, raws[q], bcs[q], size))


# ---- 6. refusals: on the host, with nothing written ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    bc = standard_bc(0)

    def fresh(dtypes=(torch.float32,), size=size, R=2):
        dd = st.DistributedDomain(*size, group=st.make_single_group())
        dd.set_backend(backend)
        dd.set_radius(st.Radius.face_edge_corner(R, 0, 0))
        dd.set_gpus([0])
        return dd, [dd.add_data(f"u{i}", dt) for i, dt in enumerate(dtypes)]

    # one face of an axis periodic and the other not
    half = _C.BoundaryConditions()
    half.set_face(1, 0, 0, FC.mirror())
    with pytest.raises(Exception, match="periodic"):
        half.boundary()
    with pytest.raises(Exception, match="periodic"):
        _C.BoundaryConditions().set_axis(0, FC.periodic(), FC.mirror())
    dd, _ = fresh()
    with pytest.raises(Exception, match="periodic"):
        dd.set_boundary_conditions(half)
    # an override whose periodic flags differ from the grid's
    dd, (q,) = fresh()
    dd.set_boundary_conditions(standard_bc(0, periodic=(False, True, True)))
    with pytest.raises(Exception, match="periodic along other axes"):
        dd.set_boundary_conditions(q, bc)
    dd.set_boundary_conditions(q, standard_bc(1, periodic=(False, True, True)))  # the same flags: accepted
    # an int quantity under a non-Open default; the message names the way out
    dd, _ = fresh((torch.float32, torch.int32))
    dd.set_boundary_conditions(bc)
    with pytest.raises(Exception, match=r"Open faces with set_boundary_conditions\(1"):
        dd.realize()
    # a sub-domain thinner than the radius along a mirrored axis
    dd, _ = fresh(size=(2, 12, 8), R=3)
    dd.set_boundary_conditions(bc)
    with pytest.raises(Exception, match="thin"):
        dd.realize()
    thin_const = standard_bc(0)
    thin_const.set_axis(0, FC.constant(1.0), FC.constant(2.0))
    dd, _ = fresh(size=(2, 12, 8), R=3)
    dd.set_boundary_conditions(thin_const)  # constants read no interior: accepted
    dd.realize()
    # an unrealized domain, and conditions set after realize()
    dd, (q,) = fresh((torch.float32, torch.int32))[0], (0,)
    dd.set_boundary_conditions(all_faces(FC.open()))
    with pytest.raises(Exception, match="realize"):
        dd.apply_boundary()
    with pytest.raises(Exception):
        boundary_apply(dd, 0, q, bc)
    dd.realize()
    with pytest.raises(Exception, match="after realize"):
        dd.set_boundary_conditions(bc)
    with pytest.raises(Exception, match="after realize"):
        dd.set_boundary_conditions(q, bc)
    # the kernel entry refuses an int quantity and a quantity out of range before anything is written
    dd.curr(0, 0).fill_(SENTINEL)
    dd.next(0, 0).fill_(SENTINEL)
    _sync(dd)
    assert not boundary_supported(dd, 0, 1, bc) and boundary_supported(dd, 0, 0, bc)
    with pytest.raises(Exception, match="fp32 / fp64"):
        boundary_apply(dd, 0, [0, 1], [bc, bc])
    with pytest.raises(Exception, match="fp32 / fp64"):
        boundary_launch_info(dd, 0, [0, 1], [bc, bc])
    with pytest.raises(Exception, match="quantity"):
        boundary_apply(dd, 0, [0, 7], [bc, bc])
    with pytest.raises(Exception, match="periodic"):
        boundary_apply(dd, 0, 0, half)
    dd.apply_boundary()  # every face Open: nothing to do
    _sync(dd)
    assert bool((dd.curr(0, 0) == SENTINEL).all()) and bool((dd.next(0, 0) == SENTINEL).all())


# ---- 7. the model ----
MODEL_CASES = [((24, 12, 12), [0], (1, 4, 4)), ((24, 12, 12), [0, 0], (1, 4, 4)), ((24, 12, 12), [0, 0], (100, 2, 3)),
               ((24, 12, 12), [0, 0, 0, 0], (100, 3, 2)), ((45, 12, 12), [0, 0, 0, 0], (1, 4, 4))]


@functools.lru_cache(maxsize=None)
def model_oracle(size, dtype, radius, rot, steps):
    u = global_field(size, dtype)
    w = random_weights(radius, 100 + radius)
    bc = standard_bc(rot)
    for _ in range(steps):
        u = star_step_reference(u, w, boundary=bc)
    return u


def gather_model(m, like):
    dd = m.domain
    got = torch.empty_like(like)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        got[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.interior(di).cpu()
    return got


def case_model(st, backend, size, gpus, cost, radius, dtype, rot):
    w = random_weights(radius, 100 + radius)
    bc = standard_bc(rot)
    m = st.StarStencil3D(size, w, fp64=dtype == torch.float64, gpus=gpus, backend=backend, axis_cost=cost, boundary=bc)
    assert m.domain.num_domains() == len(gpus) and not m.domain.boundary().all_periodic()
    u = global_field(size, dtype)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.run(3)
    m.synchronize()
    got, want = gather_model(m, u), model_oracle(size, dtype, radius, rot, 3)
    bad = int((got != want).sum())
    assert bad == 0 and torch.equal(got, want), f"run(3): {bad} cells differ, max {(got - want).abs().max().item()}"


def case_model_periodic_default(st, backend, radius, dtype):
    """boundary=None is the periodic model as before: the existing periodic oracle, bit for bit; and the reference's
    boundary=None branch is that oracle"""
    size = (24, 12, 12)
    w = random_weights(radius, 100 + radius)
    m = st.StarStencil3D(size, w, fp64=dtype == torch.float64, gpus=[0, 0], backend=backend, axis_cost=(1, 4, 4))
    assert m.boundary is None and m.domain.boundary().all_periodic()
    u = global_field(size, dtype)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.run(3)
    m.synchronize()
    assert torch.equal(gather_model(m, u), periodic_star_oracle(size, dtype, radius, 3))
    assert torch.equal(star_step_reference(u, w, boundary=None), star_step_reference(u, w))
    assert torch.equal(star_step_reference(u, w, boundary=_C.BoundaryConditions()), star_step_reference(u, w))


# ---- 8. physics (fp64) ----
def case_fixed_point(st, backend):
    """heat conduction between a wall at 0 and a wall at 1 (AntiMirror on the x faces, y and z periodic): the linear
    profile is the fixed point of the 7-point diffusion step, and the iteration from zero converges to it"""
    size = (8, 4, 4)
    bc = _C.BoundaryConditions()
    bc.set_axis(0, FC.antimirror(0.0), FC.antimirror(1.0))
    w = diffusion_star(2, 1.0 / 6.0)

    def profile(gz, gy, gx):
        return (gx.to(torch.float64) + 0.5) / 8 + 0 * (gy + gz)

    m = st.StarStencil3D(size, w, fp64=True, gpus=[0], backend=backend, boundary=bc)
    m.init(profile)
    exact = m.interior(0).cpu().clone()
    m.step()
    m.synchronize()
    change = (m.interior(0).cpu() - exact).abs().max().item()
    print(f"fixed point: one step changes the exact profile by {change:.3e}")
    assert change <= 1e-15, change
    m = st.StarStencil3D(size, w, fp64=True, gpus=[0], backend=backend, boundary=bc)
    m.init()
    iters, value = m.run_until(tol=1e-12, max_iters=2000, check_every=10)
    err = (m.interior(0).cpu() - exact).abs().max().item()
    print(f"fixed point: {iters} iterations, last change {value:.3e}, error {err:.3e}")
    assert iters <= 1000 and value < 1e-12, (iters, value)
    assert err <= 1e-9, err


def case_conservation(st, backend):
    """Mirror on all six faces: the symmetric star with mirrored ghost cells conserves the discrete total"""
    size = (12, 10, 8)
    m = st.StarStencil3D(size, diffusion_star(2, 1.0 / 6.0), fp64=True, gpus=[0], backend=backend,
                         boundary=all_faces(FC.mirror()))
    u = global_field(size, torch.float64)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    s0 = m.domain.reduce(0)
    m.run(20)
    m.synchronize()
    s1 = m.domain.reduce(0)
    print(f"conservation: sum {s0.sum!r} -> {s1.sum!r}, sum_abs {s0.sum_abs!r}")
    assert abs(s1.sum - s0.sum) <= 1e-12 * s0.sum_abs, (s0.sum, s1.sum, s0.sum_abs)
    assert not math.isclose(s0.sum_sq, s1.sum_sq, rel_tol=1e-3), "the field did not diffuse"
