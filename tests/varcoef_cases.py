"""Cases shared by test_varcoef.py (host backend, the plain loop) and test_gpu_varcoef.py (the HIP kernels of
csrc/src/kernels/stencil_varcoef.hip): the variable-coefficient diffusion stencil, every comparison bitwise against
stencil2_amd.ops.varcoef_step_reference (torch on the CPU, one op per rounding) unless a case says otherwise.

u is torch.rand from a seeded generator, kappa is 0.5 + torch.rand from a different seed, and shift and the three h are
four distinct seeded values in (-1, 1), so a swapped axis, a swapped field or a dropped term changes the result."""
import functools
import math

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (diffusion_varcoef, operator_varcoef, star_step_reference, star_weights, varcoef_apply,
                              varcoef_launch_info, varcoef_step_reference, varcoef_supported, varcoef_to_lists,
                              varcoef_weights)

from star_cases import MODEL_CASES, SENTINEL, SHAPES, dtype_id, sub_regions  # noqa: F401  (shared shapes)

DTYPES = [torch.float32, torch.float64]
U_SEED, K_SEED, W_SEED = 5, 23, 311
FC = _C.FaceCondition


def random_weights(seed=W_SEED):
    """shift and hx, hy, hz: four distinct values in (-1, 1)"""
    v = (torch.rand(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1).tolist()
    assert len(set(v)) == 4 and all(-1 < a < 1 and a != 0 for a in v)
    return varcoef_weights(*v)


@functools.lru_cache(maxsize=None)
def global_u(size, dtype, seed=U_SEED):
    """the seeded global (z, y, x) field of a case (shared, never modified)"""
    X, Y, Z = size
    return torch.rand((Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=dtype)


@functools.lru_cache(maxsize=None)
def global_kappa(size, dtype):
    X, Y, Z = size
    return 0.5 + torch.rand((Z, Y, X), generator=torch.Generator().manual_seed(K_SEED), dtype=dtype)


def wall_conditions(kind):
    """(boundary of u, kappa_boundary) of a named wall set; u: AntiMirror(0) / AntiMirror(1) along x, Mirror along y,
    periodic z. "default": kappa Mirror on the walls (kappa_boundary None); "constant": kappa Constant(2.0) on the low
    x face; "homogeneous": both AntiMirror values 0"""
    if kind is None:
        return None, None
    bc = _C.BoundaryConditions()
    bc.set_axis(0, FC.antimirror(0.0), FC.antimirror(0.0 if kind == "homogeneous" else 1.0))
    bc.set_axis(1, FC.mirror(), FC.mirror())
    kbc = None
    if kind == "constant":
        kbc = _C.BoundaryConditions()
        kbc.set_axis(0, FC.constant(2.0), FC.mirror())
        kbc.set_axis(1, FC.mirror(), FC.mirror())
    return bc, kbc


def mirror_twin(bc):
    from stencil2_amd.models.varcoef_model import kappa_conditions
    return kappa_conditions(bc)


@functools.lru_cache(maxsize=None)
def oracle(size, dtype, steps=1, walls=None):
    """`steps` reference steps of the case's fields with the case's weights (computed once, shared)"""
    u, k, w = global_u(size, dtype), global_kappa(size, dtype), random_weights()
    bc, kbc = wall_conditions(walls)
    if bc is not None and kbc is None:
        kbc = mirror_twin(bc)
    for _ in range(steps):
        u = varcoef_step_reference(u, k, w, boundary=bc, kappa_boundary=kbc)
    return u


def make_domain(st, backend, size, dtype, radius=1, padding=True, extra=()):
    """one sub-domain with the quantities u and kappa (and `extra` (name, dtype) quantities)"""
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius if not isinstance(radius, int) else st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus([0])
    if not padding:
        dd.set_padding(False)
    qu, qk = dd.add_data("u", dtype), dd.add_data("kappa", dtype)
    qs = [dd.add_data(n, dt) for n, dt in extra]
    dd.realize()
    return (dd, qu, qk, *qs)


def _sync(dd):
    if dd.backend() == _C.Backend.Device:
        torch.cuda.synchronize()


def set_field(dd, q, g):
    """copy the global (z, y, x) field into curr(q)'s interior (one sub-domain)"""
    t = dd.curr_interior(0, q)
    t.copy_(g.to(t.device))
    _sync(dd)


def differing(a, b):
    return int((a != b).sum())


# ---- 1. the kernel over shapes, both march directions, both buffer parities ----
def case_shape(st, backend, size, zchunk, dtype, expect_fast=None):
    dd, qu, qk = make_domain(st, backend, size, dtype)
    u, k, w = global_u(size, dtype), global_kappa(size, dtype), random_weights()
    want = oracle(size, dtype)
    for parity in (0, 1):
        assert dd.domain(0).parity() == parity
        set_field(dd, qu, u)
        set_field(dd, qk, k)
        dd.exchange()
        for alt in (True, False):
            tune = st.StencilTune()
            tune.zchunk = zchunk
            tune.alternate_z = alt
            info = varcoef_launch_info(dd, 0, qu, qk, w, tune=tune)
            if expect_fast is not None:
                assert (info["path"] == "fast") == expect_fast, info
                if zchunk:
                    assert info["zchunk"] == zchunk and info["zchunks"] == -(-size[2] // zchunk), info
            else:
                assert info["path"] == "host", info
            dd.next(0, qu).fill_(SENTINEL)
            _sync(dd)
            varcoef_apply(dd, 0, qu, qk, w, tune=tune)
            _sync(dd)
            got = dd.interior(dd.next(0, qu), 0).cpu()
            bad = differing(got, want)
            assert bad == 0 and torch.equal(got, want), (
                f"parity {parity} alternate_z {alt}: {bad} of {want.numel()} cells differ, max "
                f"{(got - want).abs().max().item()} ({info})")
        dd.swap()


def case_auto_chunk_info(st, backend):
    """(24, 12, 40) on the device: the automatic z chunk is the 16-plane minimum, so three chunks with two seams"""
    dd, qu, qk = make_domain(st, backend, (24, 12, 40), torch.float32)
    info = varcoef_launch_info(dd, 0, qu, qk, random_weights())
    assert {key: info[key] for key in ("path", "zchunk", "zchunks")} == {"path": "fast", "zchunk": 16, "zchunks": 3}, info
    assert info["blocks"] == 3, info


# ---- 2. sub-regions and untouched cells ----
def case_sub_region(st, backend, name, dtype, expect_fast=None):
    size = (37, 11, 9)
    lo, hi = sub_regions(size)[name]
    dd, qu, qk = make_domain(st, backend, size, dtype)
    u, k, w = global_u(size, dtype), global_kappa(size, dtype), random_weights()
    set_field(dd, qu, u)
    set_field(dd, qk, k)
    dd.next(0, qk).fill_(SENTINEL)  # the other buffer of kappa: never read, never written
    dd.exchange()
    nxt = dd.next(0, qu)
    nxt.fill_(SENTINEL)
    _sync(dd)
    before = [dd.curr(0, qu).cpu().clone(), dd.curr(0, qk).cpu().clone(), dd.next(0, qk).cpu().clone()]
    region = _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))
    tune = st.StencilTune()
    tune.zchunk = 4
    info = varcoef_launch_info(dd, 0, qu, qk, w, region=region, tune=tune)
    if name == "empty":
        assert info["path"] == "none", info
    elif expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    varcoef_apply(dd, 0, qu, qk, w, region=region, tune=tune)
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
    after = [dd.curr(0, qu).cpu(), dd.curr(0, qk).cpu(), dd.next(0, qk).cpu()]
    for b, a, what in zip(before, after, ("curr(u)", "curr(kappa)", "next(kappa)")):
        assert torch.equal(b, a), f"{what} changed"


# ---- 3. the unpadded layout and opaque elements ----
def case_generic_layout(st, backend, dtype):
    """an unpadded layout (rows of raw cells back to back, not 16-B aligned): the fast path refuses, one thread per
    cell computes the same"""
    size = (21, 9, 7)
    dd, qu, qk = make_domain(st, backend, size, dtype, padding=False)
    u, k, w = global_u(size, dtype), global_kappa(size, dtype), random_weights()
    set_field(dd, qu, u)
    set_field(dd, qk, k)
    info = varcoef_launch_info(dd, 0, qu, qk, w)
    assert info["path"] == ("generic" if backend == _C.Backend.Device else "host"), info
    dd.exchange()
    varcoef_apply(dd, 0, qu, qk, w)
    dd.swap()
    _sync(dd)
    assert torch.equal(dd.curr_interior(0, qu).cpu(), oracle(size, dtype))


def case_opaque_bytes(st, backend, es):
    """opaque quantities of 4- / 8-byte elements are taken as fp32 / fp64, as star_apply does"""
    size = (22, 12, 9)
    dtype = torch.float32 if es == 4 else torch.float64
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(1, 0, 0))
    dd.set_gpus([0])
    qu, qk = dd.native.add_data(es, "bu"), dd.native.add_data(es, "bk")
    dd.realize()
    d = dd.domain(0)
    u, k, w = global_u(size, dtype), global_kappa(size, dtype), random_weights()
    assert varcoef_supported(dd, 0, qu, qk)
    for q, g in ((qu, u), (qk, k)):
        d.region_from_host(_C.Dim3(1, 1, 1), d.size(), q, g.contiguous().numpy().tobytes(), True)
    dd.exchange()
    varcoef_apply(dd, 0, qu, qk, w)
    dd.swap()
    _sync(dd)
    got = torch.from_numpy(np.frombuffer(d.interior_to_host(qu), dtype=u.numpy().dtype).reshape(tuple(u.shape)).copy())
    assert torch.equal(got, oracle(size, dtype))


def case_kappa_is_u(st, backend, dtype, expect_fast=None):
    """qk == qu is allowed (only next(u) is written): the nonlinear operator with kappa = u"""
    size = (23, 12, 16)
    dd, qu, _ = make_domain(st, backend, size, dtype)
    u, w = global_u(size, dtype), random_weights()
    set_field(dd, qu, u)
    dd.exchange()
    info = varcoef_launch_info(dd, 0, qu, qu, w)
    if expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    varcoef_apply(dd, 0, qu, qu, w)
    dd.swap()
    _sync(dd)
    assert torch.equal(dd.curr_interior(0, qu).cpu(), varcoef_step_reference(u, u, w))


# ---- 4 / 5. the model: several sub-domains per GPU, walls ----
def make_model(st, backend, size, dtype, gpus, axis_cost=None, walls=None, w=None, group=None, methods=None):
    bc, kbc = wall_conditions(walls)
    kw = {} if methods is None else dict(methods=methods)
    m = st.VarCoefStencil3D(size, w if w is not None else random_weights(), fp64=dtype == torch.float64, gpus=list(gpus),
                            backend=backend, axis_cost=axis_cost, boundary=bc, kappa_boundary=kbc,
                            group=group if group is not None else st.make_single_group(), **kw)
    u, k = global_u(size, dtype), global_kappa(size, dtype)
    X, Y, Z = size
    m.set_kappa(lambda gz, gy, gx: k.to(gz.device)[gz % Z, gy % Y, gx % X])
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % Z, gy % Y, gx % X])
    return m


def gather_model(m, kappa=False):
    dd = m.domain
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=m.dtype)
    m.synchronize()
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        t = m.kappa_interior(di) if kappa else m.interior(di)
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = t.cpu()
    return out


def case_model(st, backend, size, gpus, axis_cost, dtype, n):
    m = make_model(st, backend, size, dtype, gpus, axis_cost)
    dd = m.domain
    assert dd.num_domains() == len(gpus)
    dim = dd.placement_dim()
    cut = min(range(3), key=lambda a: axis_cost[a])
    assert (dim.x, dim.y, dim.z)[cut] == len(gpus), f"cut {dim} for axis cost {axis_cost}"
    m.run(n)
    assert m.cells() == size[0] * size[1] * size[2]
    for di in range(dd.num_domains()):
        s = dd.domain(di).size()
        assert tuple(m.field(di).shape) == tuple(m.field(di, 1).shape) == (s.z + 2, s.y + 2, s.x + 2)
    got, want = gather_model(m), oracle(size, dtype, n)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), f"run({n}): {bad} cells differ, max {(got - want).abs().max().item()}"
    assert torch.equal(gather_model(m, kappa=True), global_kappa(size, dtype)), "kappa changed"


WALL_SIZE = (24, 12, 10)


def case_walls(st, backend, dtype, walls, gpus):
    m = make_model(st, backend, WALL_SIZE, dtype, gpus, walls=walls)
    assert m.domain.num_domains() == len(gpus)
    m.run(2)
    got, want = gather_model(m), oracle(WALL_SIZE, dtype, 2, walls)
    bad = differing(got, want)
    assert bad == 0 and torch.equal(got, want), f"{walls}: {bad} cells differ, max {(got - want).abs().max().item()}"


# ---- 7. a constant coefficient is a star ----
def case_constant_is_star(st, backend):
    """fp64, kappa = 0.5 everywhere: kappa(c) + kappa(n) = 1, so the operator is the star with centre
    shift - 2 (hx + hy + hz) and weights h in another summation order: equal within
    64 * 2^-53 * (|shift| + 4 sum |h_a|) * max |u| per cell (about 20 roundings on terms no larger than that), not bitwise"""
    size, dtype = (24, 12, 8), torch.float64
    dd, qu, qk = make_domain(st, backend, size, dtype)
    u, w = global_u(size, dtype), random_weights()
    set_field(dd, qu, u)
    set_field(dd, qk, torch.full_like(u, 0.5))
    dd.exchange()
    varcoef_apply(dd, 0, qu, qk, w)
    dd.swap()
    _sync(dd)
    got = dd.curr_interior(0, qu).cpu()
    shift, h = varcoef_to_lists(w)
    star = star_weights(1, shift - 2 * (h[0] + h[1] + h[2]), [h[0]] * 2, [h[1]] * 2, [h[2]] * 2)
    ref = star_step_reference(u, star)
    tol = 64 * 2.0 ** -53 * (abs(shift) + 4 * sum(abs(v) for v in h)) * float(u.abs().max())
    err = float((got - ref).abs().max())
    print(f"constant coefficient against the star: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (err, tol)
    assert torch.equal(got, varcoef_step_reference(u, torch.full_like(u, 0.5), w))


# ---- 8. symmetry ----
def case_symmetry(st, backend):
    """fp64 on (16, 10, 12) under the homogeneous walls: |x.A y - y.A x| <= 1e-12 |x.A y|, the dots by dd.reduce"""
    size, dtype = (16, 10, 12), torch.float64
    bc, _ = wall_conditions("homogeneous")
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(1, 0, 0))
    dd.set_gpus([0])
    qx, qy, qk = (dd.add_data(n, dtype) for n in ("x", "y", "kappa"))
    dd.set_boundary_conditions(bc)
    dd.set_boundary_conditions(qk, mirror_twin(bc))
    dd.realize()
    set_field(dd, qx, global_u(size, dtype))
    set_field(dd, qy, global_u(size, dtype, seed=U_SEED + 1))
    set_field(dd, qk, global_kappa(size, dtype))
    dd.exchange()
    dd.apply_boundary()
    w = random_weights()
    varcoef_apply(dd, 0, qx, qk, w)  # next(x) = A x
    varcoef_apply(dd, 0, qy, qk, w)  # next(y) = A y
    _sync(dd)
    xAy = dd.reduce(qx, other=qy, curr=True, other_curr=False).dot
    yAx = dd.reduce(qy, other=qx, curr=True, other_curr=False).dot
    print(f"x.Ay {xAy!r} y.Ax {yAx!r} difference {abs(xAy - yAx):.3e}")
    assert xAy != 0 and abs(xAy - yAx) <= 1e-12 * abs(xAy), (xAy, yAx)


# ---- 9. conjugate gradients ----
CG_SIZE = (16, 10, 12)
CG_TOL = {torch.float64: 1e-8, torch.float32: 1e-5}
CG_MAX_ITERS = 400


def cg_weights():
    return varcoef_weights(0.05, -0.5, -0.65, -0.35)


def cg_walls(name):
    """"periodic"; "mixed": Mirror along x, AntiMirror(0) along y, periodic z; "antimirror": AntiMirror(0) on every
    face; "inhomogeneous": Mirror along x, AntiMirror(1.0) along y, periodic z"""
    if name == "periodic":
        return None
    bc = _C.BoundaryConditions()
    if name == "antimirror":
        for ax in range(3):
            bc.set_axis(ax, FC.antimirror(0.0), FC.antimirror(0.0))
    else:
        v = 1.0 if name == "inhomogeneous" else 0.0
        bc.set_axis(0, FC.mirror(), FC.mirror())
        bc.set_axis(1, FC.antimirror(v), FC.antimirror(v))
    return bc


@functools.lru_cache(maxsize=None)
def cg_fields(dtype):
    """(kappa, f): kappa = exp(uniform(-ln 10, ln 10)), a contrast of 100; f seeded with zero mean"""
    X, Y, Z = CG_SIZE
    g = torch.Generator().manual_seed(77)
    e = (torch.rand((Z, Y, X), generator=g, dtype=torch.float64) * 2 - 1) * math.log(10.0)
    f = torch.rand((Z, Y, X), generator=g, dtype=torch.float64)
    f = f - f.mean()
    return torch.exp(e).to(dtype), f.to(dtype)


def cg_true_residual(u, f, kappa, w, bc):
    """||f - A u||2 / ||f||2 in float64 torch (A under `bc` with kappa Mirror on its walls, inhomogeneous values
    included)"""
    kbc = None if bc is None else mirror_twin(bc)
    r = f.double() - varcoef_step_reference(u.double(), kappa.double(), w, boundary=bc, kappa_boundary=kbc)
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


def case_cg(st, backend, walls, dtype, gpus=(0,)):
    from algebra_cases import gather_solution
    w, bc, tol = cg_weights(), cg_walls(walls), CG_TOL[dtype]
    kappa, f = cg_fields(dtype)
    X, Y, Z = CG_SIZE
    m = st.StarCG(CG_SIZE, w, fp64=dtype == torch.float64, gpus=list(gpus), backend=backend, boundary=bc,
                  group=st.make_single_group(), kappa=lambda gz, gy, gx: kappa.to(gz.device)[gz % Z, gy % Y, gx % X])
    assert m.domain.num_domains() == len(gpus)
    assert (m.u, m.r, m.p, m.f, m.kappa) == (0, 1, 2, 3, 4)
    m.set_rhs(lambda gz, gy, gx: f.to(gz.device)[gz % Z, gy % Y, gx % X])
    iters, relres = m.solve(tol=tol, max_iters=CG_MAX_ITERS)
    true = cg_true_residual(gather_solution(m), f, kappa, w, bc)
    print(f"varcoef cg {walls} {dtype}: iters {iters} relres {relres:.3e} true {true:.3e}")
    assert iters < CG_MAX_ITERS and relres < tol, (iters, relres, tol)
    assert true <= 2 * tol, (true, tol)


# ---- 10. run_until ----
def case_run_until(st, backend):
    """(16, 8, 8) in fp64 under all-Mirror walls, diffusion_varcoef(0.05), kappa in [0.5, 1.5]: the steps stop changing
    u before max_iters, and no-flux walls conserve the field's sum"""
    size, dtype, tol, max_iters = (16, 8, 8), torch.float64, 1e-6, 20000
    bc = _C.BoundaryConditions()
    for ax in range(3):
        bc.set_axis(ax, FC.mirror(), FC.mirror())
    m = st.VarCoefStencil3D(size, diffusion_varcoef(0.05), fp64=True, gpus=[0], backend=backend, boundary=bc,
                            group=st.make_single_group())
    u, k = global_u(size, dtype), global_kappa(size, dtype)
    assert 0.5 <= float(k.min()) and float(k.max()) <= 1.5
    m.set_kappa(lambda gz, gy, gx: k.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % size[2], gy % size[1], gx % size[0]])
    iters, value = m.run_until(tol, max_iters, check_every=50)
    print(f"run_until: {iters} steps, last change {value:.3e}")
    assert 0 < iters < max_iters and value < tol, (iters, value)
    total, got = float(u.sum()), float(gather_model(m).sum())
    assert abs(got - total) <= 1e-10 * abs(total), (got, total)


# ---- 11. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    w = random_weights()
    dd, qu, qk, qi, qd = make_domain(st, backend, size, torch.float32, extra=(("i", torch.int32), ("d", torch.float64)))
    whole = dd.domain(0).get_compute_region()
    dd.next(0, qu).fill_(SENTINEL)
    _sync(dd)
    assert varcoef_supported(dd, 0, qu, qk)
    # an integer quantity as u or as kappa
    for a, b in ((qi, qk), (qu, qi)):
        assert not varcoef_supported(dd, 0, a, b)
        with pytest.raises(Exception, match="fp32 / fp64"):
            varcoef_apply(dd, 0, a, b, w)
        with pytest.raises(Exception, match="fp32 / fp64"):
            varcoef_launch_info(dd, 0, a, b, w)
    # an fp32 u with an fp64 kappa
    assert not varcoef_supported(dd, 0, qu, qd)
    with pytest.raises(Exception, match="element size or row pitch"):
        varcoef_apply(dd, 0, qu, qd, w)
    # in-kernel wrap
    t = st.StencilTune()
    t.wrap = 1
    with pytest.raises(Exception, match="wrap"):
        varcoef_apply(dd, 0, qu, qk, w, tune=t)
    # a region outside the compute region
    for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
        with pytest.raises(Exception, match="outside compute region"):
            varcoef_apply(dd, 0, qu, qk, w, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
        with pytest.raises(Exception, match="outside compute region"):
            varcoef_launch_info(dd, 0, qu, qk, w, region=_C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi)))
    # an empty region is a no-op
    assert varcoef_launch_info(dd, 0, qu, qk, w, region=_C.Rect3(whole.lo, whole.lo))["path"] == "none"
    varcoef_apply(dd, 0, qu, qk, w, region=_C.Rect3(whole.lo, whole.lo))
    # nothing above wrote anything
    _sync(dd)
    assert bool((dd.next(0, qu) == SENTINEL).all())
    # a face radius of 0: one face short is enough
    r = st.Radius.face_edge_corner(1, 0, 0)
    r.set_dir(0, -1, 0, 0)
    dd0, qu0, qk0 = make_domain(st, backend, size, torch.float32, radius=r)
    dd0.next(0, qu0).fill_(SENTINEL)
    _sync(dd0)
    assert not varcoef_supported(dd0, 0, qu0, qk0)
    with pytest.raises(Exception, match="face radii"):
        varcoef_apply(dd0, 0, qu0, qk0, w)
    _sync(dd0)
    assert bool((dd0.next(0, qu0) == SENTINEL).all())
    # an unrealized domain has no sub-domain to apply to
    ddu = st.DistributedDomain(*size, group=st.make_single_group())
    ddu.set_backend(backend)
    ddu.add_data("u", torch.float32)
    with pytest.raises(Exception):
        varcoef_apply(ddu, 0, 0, 0, w, region=whole)
    # Open faces, in the model and in StarCG; kappa= with star weights; VarCoefWeights without kappa=
    for ax in range(3):
        bc = _C.BoundaryConditions()
        bc.set_axis(ax, FC.mirror(), FC.open())
        kbc = _C.BoundaryConditions()
        kbc.set_axis(ax, FC.open(), FC.mirror())
        mir = _C.BoundaryConditions()
        mir.set_axis(ax, FC.mirror(), FC.mirror())
        kw = dict(gpus=[0], backend=backend, group=st.make_single_group())
        with pytest.raises(ValueError, match="Open"):
            st.VarCoefStencil3D(size, w, boundary=bc, **kw)
        with pytest.raises(ValueError, match="Open"):
            st.VarCoefStencil3D(size, w, boundary=mir, kappa_boundary=kbc, **kw)
        with pytest.raises(ValueError, match="Open"):
            st.StarCG(size, w, boundary=bc, kappa=lambda gz, gy, gx: 1.0 + 0 * (gz + gy + gx), **kw)
        with pytest.raises(ValueError, match="Open"):
            st.StarCG(size, w, boundary=mir, kappa_boundary=kbc, kappa=lambda gz, gy, gx: 1.0 + 0 * (gz + gy + gx), **kw)
    kw = dict(gpus=[0], backend=backend, group=st.make_single_group())
    with pytest.raises(ValueError, match="kappa"):
        st.StarCG(size, star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]),
                  kappa=lambda gz, gy, gx: 1.0 + 0 * (gz + gy + gx), **kw)
    with pytest.raises(ValueError, match="kappa"):
        st.StarCG(size, w, **kw)
    with pytest.raises(ValueError, match="VarCoefWeights"):
        st.VarCoefStencil3D(size, star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]), **kw)


# ---- 12. builders ----
def case_builders_exact():
    w = varcoef_weights(0.25, 1, 2, 3)
    assert varcoef_to_lists(w) == (0.25, [1.0, 2.0, 3.0]) and w.shift == 0.25 and list(w.h) == [1.0, 2.0, 3.0]
    s, h = varcoef_to_lists(random_weights())
    assert varcoef_to_lists(varcoef_weights(s, *h)) == (s, h)
    assert "VarCoefWeights" in repr(w) and "0.25" in repr(w)
    # h[a] = alpha / (2 h_a^2): spacings (0.5, 2, 1) are exact in binary
    assert varcoef_to_lists(diffusion_varcoef(0.25, spacing=(0.5, 2, 1))) == (1.0, [0.5, 0.03125, 0.125])
    assert varcoef_to_lists(diffusion_varcoef(0.25)) == (1.0, [0.125, 0.125, 0.125])
    # sigma - div(kappa grad): h[a] = -1 / (2 h_a^2)
    assert varcoef_to_lists(operator_varcoef(3.0, spacing=(0.5, 2, 1))) == (3.0, [-2.0, -0.125, -0.5])
    assert varcoef_to_lists(operator_varcoef(0.0)) == (0.0, [-0.5, -0.5, -0.5])
    for bad in (0.0, (1, 2), (1, -1, 1)):
        with pytest.raises(ValueError):
            diffusion_varcoef(0.1, spacing=bad)
    with pytest.raises(Exception):
        w.h = [1.0, 2.0]
