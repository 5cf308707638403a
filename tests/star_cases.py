"""Cases shared by test_star.py (host backend, the plain loop) and test_gpu_star.py (the HIP kernels of
csrc/src/kernels/stencil_star.hip): weighted star stencils of radius 1-3, every comparison bitwise against
stencil2_amd.ops.star_step_reference (torch on the CPU, one op per product and per sum).

Fields are torch.rand from a seeded generator; weights are 6R+1 distinct seeded values in (-1, 1), so a swapped,
dropped or mis-ordered neighbour changes the result."""
import functools
import math

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (astaroth_step_reference, diffusion_star, laplacian_star, star_apply, star_launch_info,
                              star_step_reference, star_supported, star_to_lists, star_weights)

SENTINEL = -777.25  # exactly representable in fp32 and fp64; no stencil of values in [0, 1) produces it by chance

# (x, y, z), tune.zchunk (0 = automatic)
SHAPES = [
    # x and chunk remainders
    ((20, 13, 17), 0), ((21, 12, 16), 0), ((22, 12, 16), 0), ((23, 12, 16), 0),
    # the wave boundary and the second wave in x
    ((255, 12, 16), 0), ((256, 12, 16), 0), ((257, 12, 16), 0), ((513, 12, 16), 0),
    # rows per block in y (16 rows per block)
    ((24, 15, 16), 0), ((24, 16, 16), 0), ((24, 17, 16), 0), ((24, 33, 16), 0),
    # the z ring and chunk seams. tune.zchunk is taken as given (the 16-plane minimum holds for the automatic chunk
    # only), so zchunk 5 gives chunks of 5, 5, 5 and 2 planes: a chunk shorter than the ring's 2R + 1 planes at R = 3
    # and marches in both directions; zchunk 1 is the shortest chunk there is (every plane its own march)
    ((24, 12, 7), 0), ((24, 12, 8), 0), ((24, 12, 17), 5), ((24, 12, 9), 1),
    # the automatic chunk: 16-plane minimum -> chunks of 16, 16 and 8 planes
    ((24, 12, 40), 0),
]
RADII = [1, 2, 3]
DTYPES = [torch.float32, torch.float64]


def dtype_id(dt):
    return str(dt).split(".")[-1]


def random_weights(radius, seed):
    """6R+1 distinct values in (-1, 1)"""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(6 * radius + 1, generator=g, dtype=torch.float64) * 2 - 1).tolist()
    assert len(set(v)) == len(v) and all(-1 < a < 1 and a != 0 for a in v)
    r = radius
    return star_weights(radius, v[0], v[1:1 + 2 * r], v[1 + 2 * r:1 + 4 * r], v[1 + 4 * r:])


@functools.lru_cache(maxsize=None)
def global_field(size, dtype, scale=1.0, seed=5):
    """the seeded global (z, y, x) field of a case (shared, never modified)"""
    X, Y, Z = size
    return torch.rand((Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=dtype) * scale


@functools.lru_cache(maxsize=None)
def oracle(size, dtype, radius, steps=1, scale=1.0):
    """`steps` reference steps of the case's field with the case's weights (computed once, shared)"""
    u = global_field(size, dtype, scale)
    w = random_weights(radius, 100 + radius)
    for _ in range(steps):
        u = star_step_reference(u, w)
    return u


def make_domain(st, backend, size, radius, dtype, gpus=(0,), axis_cost=None, extra_int=False):
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius if not isinstance(radius, int) else st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus(list(gpus))
    if axis_cost is not None:
        dd.set_axis_cost(st.Dim3(*axis_cost))
    q = dd.add_data("u", dtype)
    if extra_int:
        dd.add_data("i", torch.int32)
    dd.realize()
    assert dd.num_domains() == len(gpus)
    return dd, q


def set_field(dd, q, u):
    """copy the global (z, y, x) field into every sub-domain's interior"""
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        t = dd.curr_interior(di, q)
        t.copy_(u[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x].to(t.device))
    _sync(dd)


def gather(dd, q, shape_like):
    out = torch.empty_like(shape_like)
    _sync(dd)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = dd.curr_interior(di, q).cpu()
    return out


def _sync(dd):
    if dd.backend() == _C.Backend.Device:
        torch.cuda.synchronize()


def differing(a, b):
    """cells that differ bitwise (NaN compares equal to NaN of the same bits: none occur in these cases)"""
    return int((a != b).sum())


# ---- 1. the kernel over shapes ----
def case_shape(st, backend, size, zchunk, radius, dtype, expect_fast=None, scale=1.0):
    dd, q = make_domain(st, backend, size, radius, dtype)
    u = global_field(size, dtype, scale)
    w = random_weights(radius, 100 + radius)
    set_field(dd, q, u)
    tune = st.StencilTune()
    tune.zchunk = zchunk
    info = star_launch_info(dd, 0, q, w, tune=tune)
    if expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
        if zchunk:
            assert info["zchunk"] == zchunk and info["zchunks"] == -(-size[2] // zchunk), info
    else:
        assert info["path"] == "host", info
    dd.exchange()
    star_apply(dd, 0, q, w, tune=tune)
    dd.swap()
    got = gather(dd, q, u)
    want = oracle(size, dtype, radius, 1, scale)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), (f"{bad} of {want.numel()} cells differ, max "
                                                 f"{(got - want).abs().max().item()} ({info})")
    return info


TINY = {torch.float32: 1e-38, torch.float64: 1e-308}


def case_tiny(st, backend, radius, dtype, scale, expect_fast=None):
    """the field scaled by 1e-33 (fp32 products of a weight and a cell below 1.2e-5 are subnormal: a few per sweep) and
    by the smallest normal magnitude of the type (nearly every product is subnormal)"""
    size = (24, 12, 8)
    if scale == TINY[dtype]:
        u, w = global_field(size, dtype, scale), random_weights(radius, 100 + radius)
        prod = (u * torch.tensor(w.center, dtype=torch.float64).to(dtype)).abs()
        n = int(((prod > 0) & (prod < torch.finfo(dtype).tiny)).sum())
        assert n > u.numel() // 2, f"only {n} subnormal products in this case"
    case_shape(st, backend, size, 0, radius, dtype, expect_fast, scale=scale)


def case_auto_chunk_info(st, backend):
    """(24, 12, 40) on the device: the automatic z chunk is the 16-plane minimum, so three chunks with two seams"""
    dd, q = make_domain(st, backend, (24, 12, 40), 3, torch.float32)
    info = star_launch_info(dd, 0, q, random_weights(3, 103))
    assert info == {"path": "fast", "zchunk": 16, "zchunks": 3, "blocks": 3}, info


def case_generic_layout(st, backend, radius, dtype):
    """an unpadded layout (rows of raw cells back to back, not 16-B aligned): the fast path refuses, one thread per
    cell computes the same"""
    size = (21, 9, 7)
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus([0])
    dd.set_padding(False)
    q = dd.add_data("u", dtype)
    dd.realize()
    u, w = global_field(size, dtype), random_weights(radius, 100 + radius)
    set_field(dd, q, u)
    info = star_launch_info(dd, 0, q, w)
    assert info["path"] == ("generic" if backend == _C.Backend.Device else "host"), info
    dd.exchange()
    star_apply(dd, 0, q, w)
    dd.swap()
    assert torch.equal(gather(dd, q, u), oracle(size, dtype, radius))


def case_opaque_bytes(st, backend, es):
    """an opaque quantity of 4- / 8-byte elements is taken as fp32 / fp64, as stencil7_apply does"""
    size, radius = (22, 12, 9), 2
    dtype = torch.float32 if es == 4 else torch.float64
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus([0])
    q = dd.native.add_data(es, "b")
    dd.realize()
    d = dd.domain(0)
    u, w = global_field(size, dtype), random_weights(radius, 100 + radius)
    assert star_supported(dd, 0, q, w)
    d.region_from_host(_C.Dim3(radius, radius, radius), d.size(), q, u.contiguous().numpy().tobytes(), True)
    dd.exchange()
    star_apply(dd, 0, q, w)
    dd.swap()
    _sync(dd)
    import numpy as np
    got = torch.from_numpy(np.frombuffer(d.interior_to_host(q), dtype=u.numpy().dtype).reshape(tuple(u.shape)).copy())
    assert torch.equal(got, oracle(size, dtype, radius))


# ---- 2. sub-regions and untouched cells ----
def sub_regions(size):
    X, Y, Z = size
    return {
        "unaligned_x": ((3, 1, 2), (X - 2, Y - 1, Z - 1)),
        "unaligned_x_odd_end": ((5, 0, 0), (18, Y, Z)),
        "thin_x": ((7, 0, 0), (8, Y, Z)),
        "thin_y": ((0, 4, 0), (X, 5, Z)),
        "thin_z": ((0, 0, 3), (X, Y, 4)),
        "one_cell": ((9, 5, 2), (10, 6, 3)),
        "empty": ((4, 4, 4), (4, 9, 7)),
    }


def case_sub_region(st, backend, name, radius, dtype, expect_fast=None):
    size = (37, 11, 9)
    lo, hi = sub_regions(size)[name]
    dd, q = make_domain(st, backend, size, radius, dtype)
    u, w = global_field(size, dtype), random_weights(radius, 100 + radius)
    set_field(dd, q, u)
    dd.exchange()
    nxt = dd.next(0, q)
    nxt.fill_(SENTINEL)
    _sync(dd)
    region = _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))
    tune = st.StencilTune()
    tune.zchunk = 4
    info = star_launch_info(dd, 0, q, w, region=region, tune=tune)
    if name == "empty":
        assert info["path"] == "none", info
    elif expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    star_apply(dd, 0, q, w, region=region, tune=tune)
    _sync(dd)
    got = nxt.cpu()  # the whole raw allocation, halo included
    want = torch.full_like(got, SENTINEL)
    ref = oracle(size, dtype, radius)
    r = radius
    want[r + lo[2]:r + hi[2], r + lo[1]:r + hi[1], r + lo[0]:r + hi[0]] = ref[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    inside = torch.zeros_like(got, dtype=torch.bool)
    inside[r + lo[2]:r + hi[2], r + lo[1]:r + hi[1], r + lo[0]:r + hi[0]] = True
    assert int(((got != want) & ~inside).sum()) == 0, "cells outside the region were written"
    assert int(((got != want) & inside).sum()) == 0, "cells of the region differ from the oracle"
    assert torch.equal(got, want)


# ---- 3. halos are read at depth R: several sub-domains on one GPU through the model ----
MODEL_CASES = [
    # size, gpus, axis_cost (the cheapest axis is cut)
    ((40, 24, 20), [0, 0], (1, 4, 4)), ((40, 24, 20), [0, 0], (100, 2, 3)), ((40, 24, 20), [0, 0], (100, 3, 2)),
    ((48, 24, 24), [0, 0, 0, 0], (1, 4, 4)), ((40, 32, 20), [0, 0, 0, 0], (100, 2, 3)),
    ((40, 24, 32), [0, 0, 0, 0], (100, 3, 2)),
    ((45, 30, 20), [0, 0], (1, 4, 4)),  # ragged: 23 + 22 cells along x
]


def case_model(st, backend, size, gpus, axis_cost, radius, dtype, n):
    w = random_weights(radius, 100 + radius)
    m = st.StarStencil3D(size, w, fp64=dtype == torch.float64, gpus=gpus, backend=backend, axis_cost=axis_cost)
    dd = m.domain
    assert dd.num_domains() == len(gpus)
    dim = dd.placement_dim()
    cut = min(range(3), key=lambda a: axis_cost[a])
    assert (dim.x, dim.y, dim.z)[cut] == len(gpus), f"cut {dim} for axis cost {axis_cost}"
    u = global_field(size, dtype)
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.run(n)
    m.synchronize()
    assert m.cells() == size[0] * size[1] * size[2]
    got = torch.empty_like(u)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        assert tuple(m.field(di).shape) == (s.z + 2 * radius, s.y + 2 * radius, s.x + 2 * radius)
        got[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.interior(di).cpu()
    want = oracle(size, dtype, radius, n)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), f"run({n}): {bad} cells differ, max {(got - want).abs().max().item()}"


# ---- 4. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    w1, w2, w3 = (random_weights(r, 100 + r) for r in (1, 2, 3))
    dd, q = make_domain(st, backend, size, 2, torch.float32, extra_int=True)
    qi = q + 1
    whole = dd.domain(0).get_compute_region()
    # the domain's radius is below R
    assert star_supported(dd, 0, q, w1) and star_supported(dd, 0, q, w2) and not star_supported(dd, 0, q, w3)
    with pytest.raises(Exception, match="face radii"):
        star_apply(dd, 0, q, w3)
    # one face short is enough
    r = st.Radius.face_edge_corner(2, 0, 0)
    r.set_dir(0, -1, 0, 1)
    dd1, q1 = make_domain(st, backend, size, r, torch.float32)
    assert star_supported(dd1, 0, q1, w1) and not star_supported(dd1, 0, q1, w2)
    with pytest.raises(Exception, match="face radii"):
        star_apply(dd1, 0, q1, w2)
    # an integer quantity
    assert not star_supported(dd, 0, qi, w1)
    with pytest.raises(Exception, match="fp32 / fp64"):
        star_apply(dd, 0, qi, w1)
    # R = 0 or 4
    for bad_r in (0, 4):
        wb = _C.StarWeights()
        wb.radius = bad_r
        assert not star_supported(dd, 0, q, wb)
        with pytest.raises(Exception, match="radius"):
            star_apply(dd, 0, q, wb)
        with pytest.raises(ValueError):
            star_weights(bad_r, 0.0, [0.0] * 2 * bad_r, [0.0] * 2 * bad_r, [0.0] * 2 * bad_r)
    # in-kernel wrap
    t = st.StencilTune()
    t.wrap = 1
    with pytest.raises(Exception, match="wrap"):
        star_apply(dd, 0, q, w1, tune=t)
    # a region outside the compute region
    for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
        with pytest.raises(Exception, match="outside compute region"):
            star_apply(dd, 0, q, w1, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
        with pytest.raises(Exception, match="outside compute region"):
            star_launch_info(dd, 0, q, w1, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
    # nothing above wrote anything
    dd.next(0, q).fill_(SENTINEL)
    star_apply(dd, 0, q, w1, region=_C.Rect3(whole.lo, whole.lo))
    _sync(dd)
    assert bool((dd.next(0, q) == SENTINEL).all())


# ---- 5. builders ----
def case_builders_exact():
    for order in (2, 4, 6):
        w = laplacian_star(order)
        r, c, x, y, z = star_to_lists(w)
        assert r == order // 2 and len(x) == len(y) == len(z) == 2 * r
        vals = [c] + x + y + z
        # each axis's coefficients sum to zero exactly in rationals; the doubles' rounding errors (2^-53 relative per
        # coefficient, two additions for the centre) leave their exact sum within 1e-15 of the largest coefficient
        assert abs(math.fsum(vals)) <= 1e-15 * max(abs(v) for v in vals), (order, math.fsum(vals))
        for ax in (x, y, z):
            assert ax == ax[::-1], f"order {order}: not symmetric: {ax}"
        assert x == y == z
    assert star_to_lists(laplacian_star(2)) == (1, -6.0, [1.0, 1.0], [1.0, 1.0], [1.0, 1.0])
    assert star_to_lists(laplacian_star(4))[2] == [-1.0 / 12.0, 4.0 / 3.0, 4.0 / 3.0, -1.0 / 12.0]
    assert star_to_lists(laplacian_star(6))[2] == [1.0 / 90.0, -3.0 / 20.0, 3.0 / 2.0, 3.0 / 2.0, -3.0 / 20.0, 1.0 / 90.0]
    # spacing: divided by h^2 per axis, the centre terms summed
    r, c, x, y, z = star_to_lists(laplacian_star(2, spacing=(0.5, 2, 1)))
    assert (x, y, z) == ([4.0, 4.0], [0.25, 0.25], [1.0, 1.0]) and c == -8.0 - 0.5 - 2.0
    # star_weights: offsets -R..-1, +1..+R
    w = star_weights(2, 9.0, [1, 2, 3, 4], [5, 6, 7, 8], [10, 11, 12, 13])
    assert [w.get(0, 0, 2), w.get(0, 0, 1), w.get(0, 1, 1), w.get(0, 1, 2)] == [1, 2, 3, 4]
    assert w.get(2, 0, 2) == 10 and w.get(2, 1, 2) == 13 and w.center == 9.0
    assert star_to_lists(w) == (2, 9.0, [1, 2, 3, 4], [5, 6, 7, 8], [10, 11, 12, 13])
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            star_weights(2, 0.0, bad, [1, 2, 3, 4], [1, 2, 3, 4])
        with pytest.raises(ValueError):
            star_weights(2, 0.0, [1, 2, 3, 4], [1, 2, 3, 4], bad)
    for bad_order in (0, 1, 3, 8):
        with pytest.raises(ValueError):
            laplacian_star(bad_order)
    d = star_to_lists(diffusion_star(2, 0.125))
    assert d == (1, 1.0 - 0.75, [0.125, 0.125], [0.125, 0.125], [0.125, 0.125])


def case_laplacian_order(st, backend):
    """fp64 sin(2 pi x / X), X = 64: the error against -(2 pi / X)^2 sin shrinks with the order"""
    import math
    size = (64, 8, 8)
    k = 2 * math.pi / size[0]
    errs = {}
    for order in (2, 4, 6):
        w = laplacian_star(order)
        dd, q = make_domain(st, backend, size, order // 2, torch.float64)
        dd.fill_from_global(q, lambda gz, gy, gx: torch.sin(k * gx.to(torch.float64)) + 0 * (gy + gz))
        dd.exchange()
        star_apply(dd, 0, q, w)
        dd.swap()
        _sync(dd)
        x = torch.arange(size[0], dtype=torch.float64).view(1, 1, -1)
        exact = (-(k * k) * torch.sin(k * x)).expand(size[2], size[1], size[0])
        errs[order] = (dd.curr_interior(0, q).cpu() - exact).abs().max().item()
    assert errs[2] > errs[4] > errs[6], errs
    return errs


def case_diffusion_vs_astaroth(st, backend):
    """identity + (1/6) Laplacian is the 6-neighbour mean: the same operator as the Astaroth proxy in another
    summation order, so equal to 1e-12 relative in fp64 (not bitwise)"""
    size = (24, 12, 8)
    w = diffusion_star(2, 1.0 / 6.0)
    dd, q = make_domain(st, backend, size, 1, torch.float64)
    u = global_field(size, torch.float64)
    set_field(dd, q, u)
    dd.exchange()
    star_apply(dd, 0, q, w)
    dd.swap()
    got = gather(dd, q, u)
    ref = astaroth_step_reference(u)
    assert ((got - ref).abs() <= 1e-12 * ref.abs()).all(), ((got - ref).abs() / ref.abs()).max().item()
    assert torch.equal(got, star_step_reference(u, w))
