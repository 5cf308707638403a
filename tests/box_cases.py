"""Cases shared by test_box.py (host backend, the plain loop) and test_gpu_box.py (the HIP kernels of
csrc/src/kernels/stencil_box.hip): weighted 27-point box stencils, every comparison bitwise against
stencil2_amd.ops.box_step_reference (torch on the CPU, one op per product and per sum) unless stated.

Fields are torch.rand from a seeded generator; weights are 27 distinct seeded values in (-1, 1), none of them 0, so a
swapped, dropped or mis-ordered neighbour changes the result. The shapes, regions and model cases are the star's
(star_cases.py): the kernel geometry is shared."""
import functools
import itertools
import math

import pytest
import torch

import algebra_cases as ac
import star_cases as sc
from stencil2_amd import _C
from stencil2_amd.ops import (axpby_reference, box_apply, box_from_star, box_launch_info, box_step_reference,
                              box_supported, box_to_lists, box_weights, diffusion_box, laplacian_box, laplacian_star,
                              smoothing_box, star_step_reference)

SENTINEL = sc.SENTINEL
SHAPES = sc.SHAPES
DTYPES = sc.DTYPES
dtype_id = sc.dtype_id
global_field = sc.global_field
set_field = sc.set_field
gather = sc.gather
differing = sc.differing
sub_regions = sc.sub_regions
_sync = sc._sync
OFFS = (-1, 0, 1)
WSEED = 127


def random_box(seed=WSEED):
    """27 distinct values in (-1, 1), none 0"""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(27, generator=g, dtype=torch.float64) * 2 - 1).tolist()
    assert len(set(v)) == 27 and all(-1 < a < 1 and a != 0 for a in v)
    return box_weights([[v[9 * k + 3 * j:9 * k + 3 * j + 3] for j in range(3)] for k in range(3)])


@functools.lru_cache(maxsize=None)
def oracle(size, dtype, steps=1, scale=1.0):
    """`steps` reference steps of the case's field with the case's weights (computed once, shared)"""
    u = global_field(size, dtype, scale)
    w = random_box()
    for _ in range(steps):
        u = box_step_reference(u, w)
    return u


def box_radius(st):
    return st.Radius.face_edge_corner(1, 1, 1)


def make_domain(st, backend, size, dtype, radius=None, **kw):
    return sc.make_domain(st, backend, size, radius if radius is not None else box_radius(st), dtype, **kw)


# ---- 1. the kernel over shapes ----
def case_shape(st, backend, size, zchunk, dtype, expect_fast=None, scale=1.0):
    dd, q = make_domain(st, backend, size, dtype)
    u = global_field(size, dtype, scale)
    w = random_box()
    set_field(dd, q, u)
    tune = st.StencilTune()
    tune.zchunk = zchunk
    info = box_launch_info(dd, 0, q, w, tune=tune)
    if expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
        if zchunk:
            assert info["zchunk"] == zchunk and info["zchunks"] == -(-size[2] // zchunk), info
    else:
        assert info["path"] == "host", info
    dd.exchange()
    box_apply(dd, 0, q, w, tune=tune)
    dd.swap()
    got = gather(dd, q, u)
    want = oracle(size, dtype, 1, scale)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), (f"{bad} of {want.numel()} cells differ, max "
                                                 f"{(got - want).abs().max().item()} ({info})")
    return info


TINY = sc.TINY


def case_tiny(st, backend, dtype, scale, expect_fast=None):
    """the star's two scales: 1e-33 (a few subnormal fp32 products per sweep) and the smallest normal magnitude of the
    type (nearly every product is subnormal)"""
    size = (24, 12, 8)
    if scale == TINY[dtype]:
        u, w = global_field(size, dtype, scale), random_box()
        prod = (u * torch.tensor(w.get(0, 0, 0), dtype=torch.float64).to(dtype)).abs()
        n = int(((prod > 0) & (prod < torch.finfo(dtype).tiny)).sum())
        assert n > u.numel() // 2, f"only {n} subnormal products in this case"
    case_shape(st, backend, size, 0, dtype, expect_fast, scale=scale)


def case_auto_chunk_info(st, backend):
    """(24, 12, 40) on the device: the automatic z chunk is the 16-plane minimum, so three chunks with two seams"""
    dd, q = make_domain(st, backend, (24, 12, 40), torch.float32)
    info = box_launch_info(dd, 0, q, random_box())
    assert info == {"path": "fast", "zchunk": 16, "zchunks": 3, "blocks": 3}, info


def case_march_direction(st, backend, dtype):
    """(24, 12, 17) with zchunk 5 (four chunks, the last of 2 planes): alternate_z on and off, on both buffer parities,
    all bitwise equal: dz = -1 is summed first, so the device kernel marches upwards whatever alternate_z says"""
    size = (24, 12, 17)
    w = random_box()
    u = global_field(size, dtype)
    outs = []
    for alt in (True, False):
        dd, q = make_domain(st, backend, size, dtype)
        set_field(dd, q, u)
        tune = st.StencilTune()
        tune.zchunk = 5
        tune.alternate_z = alt
        for _ in range(2):  # the second step runs on the odd parity, where alternate_z would flip a march
            dd.exchange()
            box_apply(dd, 0, q, w, tune=tune)
            dd.swap()
        outs.append(gather(dd, q, u))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], oracle(size, dtype, 2))


def case_generic_layout(st, backend, dtype):
    """an unpadded layout (rows of raw cells back to back, not 16-B aligned): the fast path refuses, one thread per
    cell computes the same"""
    size = (21, 9, 7)
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(box_radius(st))
    dd.set_gpus([0])
    dd.set_padding(False)
    q = dd.add_data("u", dtype)
    dd.realize()
    u, w = global_field(size, dtype), random_box()
    set_field(dd, q, u)
    info = box_launch_info(dd, 0, q, w)
    assert info["path"] == ("generic" if backend == _C.Backend.Device else "host"), info
    dd.exchange()
    box_apply(dd, 0, q, w)
    dd.swap()
    assert torch.equal(gather(dd, q, u), oracle(size, dtype))


def case_opaque_bytes(st, backend, es):
    """an opaque quantity of 4- / 8-byte elements is taken as fp32 / fp64, as stencil7_apply does"""
    size = (22, 12, 9)
    dtype = torch.float32 if es == 4 else torch.float64
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(box_radius(st))
    dd.set_gpus([0])
    q = dd.native.add_data(es, "b")
    dd.realize()
    d = dd.domain(0)
    u, w = global_field(size, dtype), random_box()
    assert box_supported(dd, 0, q)
    d.region_from_host(_C.Dim3(1, 1, 1), d.size(), q, u.contiguous().numpy().tobytes(), True)
    dd.exchange()
    box_apply(dd, 0, q, w)
    dd.swap()
    _sync(dd)
    import numpy as np
    got = torch.from_numpy(np.frombuffer(d.interior_to_host(q), dtype=u.numpy().dtype).reshape(tuple(u.shape)).copy())
    assert torch.equal(got, oracle(size, dtype))


# ---- 2. sub-regions and untouched cells ----
def case_sub_region(st, backend, name, dtype, expect_fast=None):
    size = (37, 11, 9)
    lo, hi = sub_regions(size)[name]
    dd, q = make_domain(st, backend, size, dtype)
    u, w = global_field(size, dtype), random_box()
    set_field(dd, q, u)
    dd.exchange()
    nxt = dd.next(0, q)
    nxt.fill_(SENTINEL)
    _sync(dd)
    region = _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))
    tune = st.StencilTune()
    tune.zchunk = 4
    info = box_launch_info(dd, 0, q, w, region=region, tune=tune)
    if name == "empty":
        assert info["path"] == "none", info
    elif expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    box_apply(dd, 0, q, w, region=region, tune=tune)
    _sync(dd)
    got = nxt.cpu()  # the whole raw allocation, halo included
    want = torch.full_like(got, SENTINEL)
    ref = oracle(size, dtype)
    want[1 + lo[2]:1 + hi[2], 1 + lo[1]:1 + hi[1], 1 + lo[0]:1 + hi[0]] = ref[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    inside = torch.zeros_like(got, dtype=torch.bool)
    inside[1 + lo[2]:1 + hi[2], 1 + lo[1]:1 + hi[1], 1 + lo[0]:1 + hi[0]] = True
    assert int(((got != want) & ~inside).sum()) == 0, "cells outside the region were written"
    assert int(((got != want) & inside).sum()) == 0, "cells of the region differ from the oracle"
    assert torch.equal(got, want)


# ---- 3. edges and corners from other sub-domains: several sub-domains on one GPU through the model ----
# size, gpus, axis_cost (None: the default placement), expected placement (None: the cheapest axis holds every cut)
# (the star's list ends with the ragged x cut: (45, 30, 20) as 23 + 22 cells)
MODEL_CASES = [(size, gpus, cost, None) for size, gpus, cost in sc.MODEL_CASES] + [
    ((24, 16, 16), [0] * 8, None, (2, 2, 2)),  # every corner halo comes from a different sub-domain
]


def gather_model(m, u):
    dd = m.domain
    got = torch.empty_like(u)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        assert tuple(m.field(di).shape) == (s.z + 2, s.y + 2, s.x + 2)
        got[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.interior(di).cpu()
    return got


def case_model(st, backend, size, gpus, axis_cost, placement, dtype, n):
    w = random_box()
    m = st.BoxStencil3D(size, w, fp64=dtype == torch.float64, gpus=gpus, backend=backend, axis_cost=axis_cost)
    dd = m.domain
    assert dd.num_domains() == len(gpus)
    dim = dd.placement_dim()
    if placement is not None:
        assert (dim.x, dim.y, dim.z) == placement, f"cut {dim}, expected {placement}"
    else:
        cut = min(range(3), key=lambda a: axis_cost[a])
        assert (dim.x, dim.y, dim.z)[cut] == len(gpus), f"cut {dim} for axis cost {axis_cost}"
    u = global_field(size, dtype)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.run(n)
    m.synchronize()
    assert m.cells() == size[0] * size[1] * size[2]
    got = gather_model(m, u)
    want = oracle(size, dtype, n)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), f"run({n}): {bad} cells differ, max {(got - want).abs().max().item()}"


# ---- 4. boundary conditions: composed edge and corner ghost cells are read ----
def box_walls():
    """x mirror / antimirror(0.5), y antimirror(-1) / constant(2), z mirror / mirror"""
    FC = _C.FaceCondition
    bc = _C.BoundaryConditions()
    bc.set_axis(0, FC.mirror(), FC.antimirror(0.5))
    bc.set_axis(1, FC.antimirror(-1.0), FC.constant(2.0))
    bc.set_axis(2, FC.mirror(), FC.mirror())
    return bc


BC_SIZE = (20, 12, 10)


@functools.lru_cache(maxsize=None)
def bc_oracle(dtype, steps=2):
    u, w, bc = global_field(BC_SIZE, dtype), random_box(), box_walls()
    for _ in range(steps):
        u = box_step_reference(u, w, boundary=bc)
    return u


def case_boundary(st, backend, dtype, ndom):
    size = BC_SIZE
    m = st.BoxStencil3D(size, random_box(), fp64=dtype == torch.float64, gpus=[0] * ndom, backend=backend,
                        boundary=box_walls())
    assert m.domain.num_domains() == ndom
    u = global_field(size, dtype)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.run(2)
    m.synchronize()
    got = gather_model(m, u)
    want = bc_oracle(dtype)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), f"{bad} cells differ, max {(got - want).abs().max().item()}"


# ---- 5. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    w = random_box()
    dd, q = make_domain(st, backend, size, torch.float32, extra_int=True)
    qi = q + 1
    whole = dd.domain(0).get_compute_region()
    assert box_supported(dd, 0, q)
    # corners, then edges and corners, not exchanged; one corner direction short is enough
    one = st.Radius.face_edge_corner(1, 1, 1)
    one.set_dir(1, -1, 1, 0)
    for r in (st.Radius.face_edge_corner(1, 1, 0), st.Radius.face_edge_corner(1, 0, 0), one):
        dd1, q1 = make_domain(st, backend, size, torch.float32, radius=r)
        assert not box_supported(dd1, 0, q1)
        dd1.next(0, q1).fill_(SENTINEL)
        with pytest.raises(Exception, match="radii"):
            box_apply(dd1, 0, q1, w)
        with pytest.raises(Exception, match="radii"):
            box_launch_info(dd1, 0, q1, w)
        _sync(dd1)
        assert bool((dd1.next(0, q1) == SENTINEL).all())
    dd.next(0, q).fill_(SENTINEL)
    # an integer quantity
    assert not box_supported(dd, 0, qi)
    with pytest.raises(Exception, match="fp32 / fp64"):
        box_apply(dd, 0, qi, w)
    # in-kernel wrap
    t = st.StencilTune()
    t.wrap = 1
    with pytest.raises(Exception, match="wrap"):
        box_apply(dd, 0, q, w, tune=t)
    # a region outside the compute region
    for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
        with pytest.raises(Exception, match="outside compute region"):
            box_apply(dd, 0, q, w, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
        with pytest.raises(Exception, match="outside compute region"):
            box_launch_info(dd, 0, q, w, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
    # nothing above wrote anything, nor does an empty region
    box_apply(dd, 0, q, w, region=_C.Rect3(whole.lo, whole.lo))
    _sync(dd)
    assert bool((dd.next(0, q) == SENTINEL).all())


# ---- 6. builders ----
def _flips_and_permutations(w):
    """the nested lists of w under every axis flip and axis permutation"""
    out = []
    for perm in itertools.permutations(range(3)):
        for flip in itertools.product((1, -1), repeat=3):
            def at(d):
                s = [d[perm[a]] * flip[a] for a in range(3)]
                return w[s[0] + 1][s[1] + 1][s[2] + 1]
            out.append([[[at((dz, dy, dx)) for dx in OFFS] for dy in OFFS] for dz in OFFS])
    return out


def by_class(c):
    return [[[c[abs(dz) + abs(dy) + abs(dx)] for dx in OFFS] for dy in OFFS] for dz in OFFS]


def case_builders_exact():
    x = [[[float(9 * k + 3 * j + i) + 0.5 for i in range(3)] for j in range(3)] for k in range(3)]
    b = box_weights(x)
    assert box_to_lists(b) == x
    assert b.get(-1, -1, -1) == 0.5 and b.get(-1, -1, 1) == 2.5 and b.get(-1, 1, -1) == 6.5 and b.get(1, -1, -1) == 18.5
    for bad in ([1.0] * 27, [[1.0] * 3] * 3, [[[1.0] * 3] * 3] * 2, [[[1.0] * 4] * 3] * 3, [[[1.0] * 3] * 2] * 3, 1.0):
        with pytest.raises(ValueError):
            box_weights(bad)
    pinned = {7: [-6.0, 1.0, 0.0, 0.0], 19: [-24.0 / 6.0, 2.0 / 6.0, 1.0 / 6.0, 0.0 / 6.0],
              27: [-128.0 / 30.0, 14.0 / 30.0, 3.0 / 30.0, 1.0 / 30.0]}
    for points, c in pinned.items():
        w = box_to_lists(laplacian_box(points))
        assert w == by_class(c), points
        flat = [v for p in w for r in p for v in r]
        # the classes' coefficients sum to zero exactly in rationals; the doubles' rounding errors leave their exact
        # sum within 1e-15 of the largest coefficient (the star test's bound)
        assert abs(math.fsum(flat)) <= 1e-15 * max(abs(v) for v in flat), (points, math.fsum(flat))
        # second moment 2 per axis (sum of w d_a^2), within the same bound
        for a in range(3):
            m2 = math.fsum(w[dz + 1][dy + 1][dx + 1] * (dz, dy, dx)[a] ** 2 for dz in OFFS for dy in OFFS for dx in OFFS)
            assert abs(m2 - 2.0) <= 1e-15 * max(abs(v) for v in flat), (points, a, m2)
        # spacing 0.5 multiplies every coefficient by 4 exactly
        assert box_to_lists(laplacian_box(points, spacing=0.5)) == [[[4.0 * v for v in r] for r in p] for p in w]
        d = box_to_lists(diffusion_box(points, 0.125))
        want = [[[0.125 * v for v in r] for r in p] for p in w]
        want[1][1][1] = 1.0 + want[1][1][1]
        assert d == want
    s = box_to_lists(smoothing_box())
    assert s == by_class([8.0 / 64.0, 4.0 / 64.0, 2.0 / 64.0, 1.0 / 64.0])
    assert sum(v for p in s for r in p for v in r) == 1.0  # exact in binary, in any order
    for w in [laplacian_box(p) for p in (7, 19, 27)] + [diffusion_box(27, 0.1), smoothing_box(),
                                                         box_from_star(laplacian_star(2))]:
        lists = box_to_lists(w)
        assert all(v == lists for v in _flips_and_permutations(lists))
    # the check itself sees an asymmetric box
    assert not all(v == box_to_lists(random_box()) for v in _flips_and_permutations(box_to_lists(random_box())))
    for bad_points in (0, 6, 9, 26):
        with pytest.raises(ValueError):
            laplacian_box(bad_points)
        with pytest.raises(ValueError):
            diffusion_box(bad_points, 0.1)
    for order in (4, 6):  # radius 2 and 3
        with pytest.raises(ValueError):
            box_from_star(laplacian_star(order))
    from stencil2_amd.ops import star_weights
    f = box_from_star(star_weights(1, 9.0, [1.0, 2.0], [3.0, 4.0], [5.0, 6.0]))
    assert (f.get(0, 0, 0), f.get(0, 0, -1), f.get(0, 0, 1), f.get(0, -1, 0), f.get(0, 1, 0), f.get(-1, 0, 0),
            f.get(1, 0, 0)) == (9.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    assert sum(1 for p in box_to_lists(f) for r in p for v in r if v != 0.0) == 7


def gamma(n, dtype=torch.float64):
    """gamma_n = n u / (1 - n u), u the unit roundoff of the type"""
    u = torch.finfo(dtype).eps / 2
    return n * u / (1 - n * u)


def abs_sum(u, w, boundary=None):
    """sum over d of |w_d u_d| per cell, in float64 torch"""
    lists = box_to_lists(w)
    absw = box_weights([[[abs(v) for v in r] for r in p] for p in lists])
    return box_step_reference(u.abs().double(), absw, boundary=boundary)


def run_once(st, backend, size, dtype, w, u):
    dd, q = make_domain(st, backend, size, dtype)
    set_field(dd, q, u)
    dd.exchange()
    box_apply(dd, 0, q, w)
    dd.swap()
    return gather(dd, q, u)


def case_box_from_star(st, backend):
    """box_from_star(laplacian_star(2)) against star_step_reference of the star: the same 7 non-zero terms (and 20
    exact zeros) in another order, so within the any-order bound 2 gamma_27 sum |w_d u_d| per cell; bitwise equal to
    box_step_reference"""
    size = (24, 12, 8)
    star = laplacian_star(2)
    w = box_from_star(star)
    u = global_field(size, torch.float64)
    got = run_once(st, backend, size, torch.float64, w, u)
    assert torch.equal(got, box_step_reference(u, w))
    bound = 2 * gamma(27) * abs_sum(u, w)
    err = (got - star_step_reference(u, star)).abs()
    assert bool((err <= bound).all()), (err / bound).max().item()


def case_symbol(st, backend):
    """fp64 laplacian_box(27) on u = sin(kx x) sin(ky y) sin(kz z), periodic (32, 16, 16), one period per axis: where
    |u| >= 0.1, out / u = sum_d w_d cos(kx dx) cos(ky dy) cos(kz dz) within 2 gamma_27 sum |w_d u_d| / |u|. The three
    sine tables and the symbol are computed in extended precision and rounded once, so the field's own error (a few
    units in the last place of each cell) stays far below the bound"""
    import numpy as np
    size = (32, 16, 16)
    w = laplacian_box(27)
    L = np.longdouble
    pi = L("3.14159265358979323846264338327950288")
    k = [2 * pi / L(n) for n in size]
    tab = [torch.from_numpy(np.sin(k[a] * np.arange(size[a], dtype=L)).astype(np.float64)) for a in range(3)]
    u = (tab[2].view(-1, 1, 1) * tab[1].view(1, -1, 1)) * tab[0].view(1, 1, -1)
    lam = L(0)
    for dz in OFFS:
        for dy in OFFS:
            for dx in OFFS:
                lam += L(w.get(dz, dy, dx)) * np.cos(k[0] * dx) * np.cos(k[1] * dy) * np.cos(k[2] * dz)
    lam = float(lam)
    got = run_once(st, backend, size, torch.float64, w, u)
    assert torch.equal(got, box_step_reference(u, w))
    mask = u.abs() >= 0.1
    assert int(mask.sum()) > u.numel() // 4
    bound = 2 * gamma(27) * abs_sum(u, w)[mask] / u.abs()[mask]
    err = (got[mask] / u[mask] - lam).abs()
    assert bool((err <= bound).all()), ((err / bound).max().item(), lam)
    assert -1.0 < lam < 0.0  # close to -(kx^2 + ky^2 + kz^2) = -0.347


# ---- 7. CG on boxes ----
def box_helmholtz(points):
    """I - laplacian_box(points)"""
    w = box_to_lists(laplacian_box(points))
    out = [[[-v for v in r] for r in p] for p in w]
    out[1][1][1] = 1.0 + out[1][1][1]
    return box_weights(out)


def box_poisson(points):
    """-laplacian_box(points)"""
    return box_weights([[[-v for v in r] for r in p] for p in box_to_lists(laplacian_box(points))])


CG_CASES = {
    "helmholtz_periodic": (box_helmholtz, None),
    "helmholtz_walls": (box_helmholtz, 0.0),
    "poisson_walls": (box_poisson, 0.0),
    "poisson_walls_0.25": (box_poisson, 0.25),
    "poisson_walls_1.0": (box_poisson, 1.0),
}
CG_POINTS = [19, 27]


def oracle_cg(w, bc, f, tol, max_iters):
    """the algorithm of StarCG.solve on the global grid, as algebra_cases.oracle_cg, with A through box_step_reference"""
    def ssq(v):
        return float((v.double() * v.double()).sum())

    hom = ac.homogeneous(bc)
    u = torch.zeros_like(f)
    ff = ssq(f)
    r = axpby_reference(1.0, f, -1.0, box_step_reference(u, w, boundary=bc))
    rr = ssq(r)
    p = r.clone()
    it = 0
    while it < max_iters and math.sqrt(rr / ff) >= tol:
        Ap = box_step_reference(p, w, boundary=hom)
        alpha = rr / float((p.double() * Ap.double()).sum())
        u = axpby_reference(1.0, u, alpha, p)
        r = axpby_reference(1.0, r, -alpha, Ap)
        rr_new = ssq(r)
        p = axpby_reference(1.0, r, rr_new / rr, p)
        rr = rr_new
        it += 1
    return it, math.sqrt(rr / ff), u


@functools.lru_cache(maxsize=None)
def cg_oracle(name, points, dtype):
    wf, zv = CG_CASES[name]
    it, rel, _ = oracle_cg(wf(points), None if zv is None else ac.walls(zv), ac.cg_rhs(dtype), ac.CG_TOL[dtype], 1000)
    return it, rel


def true_residual(u, f, w, bc):
    r = f.double() - box_step_reference(u.double(), w, boundary=bc)
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


def case_cg(st, backend, name, points, dtype):
    wf, zv = CG_CASES[name]
    w, bc, tol = wf(points), None if zv is None else ac.walls(zv), ac.CG_TOL[dtype]
    m, f = ac.make_cg(st, backend, w, bc, dtype)
    r = m.domain.domain(0).radius()
    assert all(r.dir(dx, dy, dz) == 1 for dx in OFFS for dy in OFFS for dz in OFFS if (dx, dy, dz) != (0, 0, 0))
    iters, relres = m.solve(tol=tol, max_iters=1000)
    want_iters, want_rel = cg_oracle(name, points, dtype)
    true = true_residual(ac.gather_solution(m), f, w, bc)
    print(f"{name} {points} {dtype}: iters {iters} relres {relres:.3e} true {true:.3e}; oracle iters {want_iters} "
          f"relres {want_rel:.3e}")
    assert relres < tol and true <= 2 * tol, (relres, true, tol)
    assert abs(iters - want_iters) <= 1, (iters, want_iters)


def case_cg_symmetry(st, backend):
    """central symmetry is enough on a periodic grid; walls also need the weights even along the walled axes; a box
    that is not centrally symmetric is always refused"""
    g = torch.Generator().manual_seed(7)
    v = (torch.rand(27, generator=g, dtype=torch.float64) * 0.1).tolist()
    w = [[[v[9 * k + 3 * j + i] for i in range(3)] for j in range(3)] for k in range(3)]
    central = [[[w[k][j][i] + w[2 - k][2 - j][2 - i] for i in range(3)] for j in range(3)] for k in range(3)]
    central[1][1][1] = 8.0
    cw = box_weights(central)
    kw = dict(backend=backend, gpus=[0], group=st.make_single_group())
    with pytest.raises(ValueError, match=r"walled axis 1: offset"):
        st.StarCG(ac.CG_SIZE, cw, boundary=ac.walls(0.0), **kw)
    m = st.StarCG(ac.CG_SIZE, cw, **kw)  # periodic: accepted, and it solves
    f = ac.cg_rhs(torch.float64)
    X, Y, Z = ac.CG_SIZE
    m.set_rhs(lambda gz, gy, gx: f.to(gz.device)[gz % Z, gy % Y, gx % X])
    iters, relres = m.solve(tol=1e-10, max_iters=200)
    assert relres < 1e-10 and true_residual(ac.gather_solution(m), f, cw, None) <= 2e-10, (iters, relres)
    # even along the walled axes y and z and centrally symmetric (hence even along x too): accepted with walls
    even = [[[central[min(k, 2 - k)][min(j, 2 - j)][min(i, 2 - i)] for i in range(3)] for j in range(3)] for k in range(3)]
    st.StarCG(ac.CG_SIZE, box_weights(even), boundary=ac.walls(0.0), **kw)
    central[0][1][2] += 0.5
    for bc in (None, ac.walls(0.0)):
        with pytest.raises(ValueError, match=r"symmetric weights: offset"):
            st.StarCG(ac.CG_SIZE, box_weights(central), boundary=bc, **kw)
    # star weights behave as before
    st.StarCG(ac.CG_SIZE, ac.helmholtz(), boundary=ac.walls(0.0), **kw)


# ---- 8. run_until ----
def case_run_until(st, backend):
    """BoxStencil3D((16, 16, 16), diffusion_box(27, 0.1), fp64) from a sine: the same (iters, value) as a torch loop
    over box_step_reference with the same check schedule (check every 10th step: the inf norm of the last step's
    change)"""
    size = (16, 16, 16)
    w = diffusion_box(27, 0.1)
    k = 2 * math.pi / 16
    z = torch.arange(16, dtype=torch.float64)
    u = (torch.sin(k * z).view(-1, 1, 1) * torch.sin(k * z).view(1, -1, 1)) * torch.sin(k * z).view(1, 1, -1)
    m = st.BoxStencil3D(size, w, fp64=True, gpus=[0], backend=backend)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % 16, gy % 16, gx % 16])
    tol, cap, every = 2e-3, 200, 10
    iters, value = m.run_until(tol, cap, check_every=every)
    it, val = 0, None
    while it < cap:
        for _ in range(every):
            prev, u = u, box_step_reference(u, w)
        it += every
        val = float((u - prev).abs().max())
        if val < tol:
            break
    assert 0 < it < cap, (it, val)
    assert (iters, value) == (it, val), ((iters, value), (it, val))
    assert torch.equal(gather_model(m, u), u)
