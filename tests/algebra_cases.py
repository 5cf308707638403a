"""Cases shared by test_algebra.py (host backend, the plain loop) and test_gpu_algebra.py (the HIP kernels of
csrc/src/kernels/field_axpby.hip): dst = a x (+ b y) bitwise against ops.axpby_reference, the stats of the stored
values fused into the same pass, DistributedDomain.axpby / copy / scale, and the StarCG solver against a torch CG.

Every launch is checked the same way (Runner.run): every byte of both buffers of the three quantities is first set to
0xAB, only the source cells of the region are written, all six buffers are read back whole before and after the call
(row padding and tails included), and afterwards the region of dst must hold the oracle's bits and every other byte of
every buffer the bits it had before.

One refusal of field_axpby cannot be provoked from Python: operands of one element size always get one row pitch."""
import functools
import math

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (axpby_reference, field_axpby, field_axpby_launch_info, field_axpby_supported,
                              field_reduce, pad_reference, star_step_reference, star_weights)

import reduce_cases as rc
from reduce_cases import exact_field, make_domain, put, random_field, rect
from star_cases import sub_regions

FILL = 0xAB
SIZES = rc.SIZES
SHAPE_CASES = rc.SHAPE_CASES
shape_id, dtype_id = rc.shape_id, rc.dtype_id
COEFFS = [(1, None), (0.375, None), (1, -0.7), (1.3, 2.9), (0, 1)]
BUFFERS = [(d, x, y) for d in (True, False) for x in (True, False) for y in (True, False)]
ALIAS_SIZES = [(37, 11, 9), (257, 3, 2)]
# name -> (dst, x, y) as (quantity letter, curr?)
ALIASES = {
    "dst_is_x": (("a", True), ("a", True), ("b", True)),
    "dst_is_y": (("a", False), ("b", True), ("a", False)),
    "dst_is_x_is_y": (("a", True), ("a", True), ("a", True)),
    "dst_other_buffer_of_x": (("a", False), ("a", True), ("b", False)),
    "dst_third_quantity": (("c", True), ("a", True), ("b", False)),
}
FORCED = rc.FORCED
RANDOM_SIZE = rc.RANDOM_SIZE
DD_SIZE = rc.DD_SIZE


def regions(size):
    r = dict(sub_regions(size))
    r["whole"] = ((0, 0, 0), tuple(size))
    return r


def np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def get(dd, q, curr, dtype):
    """the compute regions of (q, curr) of every sub-domain gathered into the global (z, y, x) tensor"""
    rc.sync(dd)
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=dtype)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s, r = d.origin(), d.size(), d.radius()
        raw = d.region_to_host(_C.Dim3(r.x(-1), r.y(-1), r.z(-1)), s, q, curr)
        part = torch.from_numpy(np.frombuffer(raw, dtype=np_dtype(dtype)).reshape(s.z, s.y, s.x).copy())
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = part
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


class Runner:
    """one sub-domain with three quantities a, b, c of one dtype, reused by the launches of a test"""

    def __init__(self, st, backend, size, dtype, opaque=0, **layout):
        self.st, self.backend, self.size, self.dtype = st, backend, tuple(size), dtype
        self.dd, qa, qb, (qc,) = make_domain(st, backend, size, dtype, opaque=opaque, extra=(dtype,), **layout)
        self.q = {"a": qa, "b": qb, "c": qc}
        self.d = self.dd.domain(0)
        self.word = np.uint32 if dtype == torch.float32 else np.uint64

    def buffers(self):
        rc.sync(self.dd)
        return {(n, c): np.frombuffer(self.d.buffer_to_host(q, c), dtype=self.word).copy()
                for n, q in self.q.items() for c in (True, False)}

    def index(self, q, lo, hi):
        p, r = self.d.pitch(q), self.d.radius()
        z = np.arange(lo[2], hi[2]).reshape(-1, 1, 1) + r.z(-1)
        y = np.arange(lo[1], hi[1]).reshape(1, -1, 1) + r.y(-1)
        x = np.arange(lo[0], hi[0]).reshape(1, 1, -1) + r.x(-1)
        return (z * p.y + y) * p.x + self.d.pad_x(q) + x

    def source(self, k, data):
        if data == "exact":
            return exact_field(self.size, 21 + k).to(self.dtype)
        return random_field(self.size, self.dtype, 61 + k)

    def run(self, a, b, dst, x, y=None, lo=(0, 0, 0), hi=None, data="random", planted=None, device_path="fast",
            stream=0, **kw):
        """field_axpby(dst <- a x + b y) over [lo, hi) with the byte check of the module docstring; operands are
        (quantity letter, curr?). Returns (what the call returned, the launch info, the oracle's region)"""
        hi = self.size if hi is None else tuple(hi)
        if b is None:
            y = None
        for n, q in self.q.items():
            self.d.fill_bytes(q, FILL, True, True)
        srcs = {}
        for op in (x, y):
            if op is not None and op not in srcs:
                u = self.source(len(srcs) + (0 if op[1] else 2), data)
                if planted and not srcs:
                    u = u.clone()
                    for (px, py, pz), v in planted.items():
                        u[pz, py, px] = v
                srcs[op] = u
                put(self.dd, self.q[op[0]], op[1], u, lo, hi)
        before = self.buffers()
        sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        want = axpby_reference(a, srcs[x][sl], b, None if y is None else srcs[y][sl])
        args = dict(dst_curr=dst[1], x_curr=x[1], y_curr=True if y is None else y[1], region=rect(lo, hi))
        qy = None if y is None else self.q[y[0]]
        bb = 0.0 if b is None else b
        info = field_axpby_launch_info(self.dd, 0, self.q[dst[0]], a, self.q[x[0]], bb, qy, **args, **kw)
        empty = any(hi[i] <= lo[i] for i in range(3))
        assert info["path"] == ("none" if empty else rc.expected_path(self.backend, device_path)), info
        if not empty:
            assert info["items"] == (hi[1] - lo[1]) * (hi[2] - lo[2]), info
            if self.backend == _C.Backend.Device:
                mb = kw.get("max_blocks", 0)
                assert info["blocks"] == mb if mb else 1 <= info["blocks"] <= info["items"], info
        assert field_axpby_supported(self.dd, 0, self.q[dst[0]], self.q[x[0]], qy)
        out = field_axpby(self.dd, 0, self.q[dst[0]], a, self.q[x[0]], bb, qy, stream=stream, **args, **kw)
        after = self.buffers()
        what = f"{self.size} {self.dtype} a={a} b={b} dst={dst} x={x} y={y} [{lo}, {hi}) {kw} {info}"
        for key, old in before.items():
            expect = old
            if key == dst and not empty:
                expect = old.copy()
                expect[self.index(self.q[dst[0]], lo, hi)] = want.numpy().view(self.word)
            diff = after[key] != expect
            if planted and key == dst:  # NaN payloads are not part of the contract
                f = np_dtype(self.dtype)
                diff &= ~(np.isnan(after[key].view(f)) & np.isnan(expect.view(f)))
            assert not diff.any(), (f"{what}: buffer {key}: {int(diff.sum())} elements differ "
                                    f"(first at element {int(np.flatnonzero(diff)[0])})")
        return out, info, want


# ---- 1. bitwise over shapes, coefficients and operand buffers ----
def case_shape(st, backend, size, dtype):
    r = Runner(st, backend, size, dtype)
    for a, b in COEFFS:
        for dc, xc, yc in BUFFERS:
            if b is None and not yc:
                continue  # no y: its buffer choice is no new case
            out, _, _ = r.run(a, b, ("a", dc), ("b", xc), ("c", yc))
            assert out is None


# ---- 2. aliasing ----
def case_alias(st, backend, size, dtype, name):
    dst, x, y = ALIASES[name]
    r = Runner(st, backend, size, dtype)
    r.run(1.3, 2.9, dst, x, y)
    r.run(1, -0.7, dst, x, y, stats=True)
    if name != "dst_is_x_is_y":
        r.run(0.375, None, dst, x)


# ---- 3. untouched bytes over sub-regions ----
def case_region(st, backend, name, dtype, stats):
    size = (37, 11, 9)
    lo, hi = regions(size)[name]
    r = Runner(st, backend, size, dtype)
    out, _, want = r.run(1.3, 2.9, ("a", False), ("b", True), ("c", True), lo, hi, stats=stats)
    r.run(0.375, None, ("a", True), ("a", True), None, lo, hi, stats=stats)  # in place
    if stats and name == "empty":
        assert rc.fields(out) == rc.IDENTITY


# ---- 4. layouts and opaque elements ----
def case_layout(st, backend, name, dtype):
    kw, path = rc.LAYOUTS[name]
    kw = dict(kw)
    if kw.get("radius") == "asym":
        kw["radius"] = rc.asymmetric_radius(st)
    r = Runner(st, backend, (37, 11, 9), dtype, **kw)
    r.run(1.3, 2.9, ("a", True), ("b", True), ("c", False), device_path=path)
    r.run(1, -0.7, ("a", True), ("a", True), ("b", True), (3, 1, 2), (35, 10, 8), device_path=path, stats=True)


def case_opaque(st, backend, es):
    r = Runner(st, backend, (37, 11, 9), torch.float32 if es == 4 else torch.float64, opaque=es)
    r.run(1.3, 2.9, ("a", True), ("b", True), ("c", False))
    r.run(1.3, 2.9, ("b", False), ("a", True), ("b", True), stats=True)


# ---- 5. forced grids ----
def case_forced_grid(st, backend, size, dtype, max_blocks):
    """same field bits (the byte check) and the same exact stats as the automatic grid"""
    r = Runner(st, backend, size, dtype)
    auto, _, _ = r.run(2, -3, ("a", True), ("b", True), ("c", False), data="exact", stats=True)
    forced, _, _ = r.run(2, -3, ("a", True), ("b", True), ("c", False), data="exact", stats=True, max_blocks=max_blocks)
    assert rc.fields(auto) == rc.fields(forced), (rc.fields(auto), rc.fields(forced))
    assert r.run(1.3, 2.9, ("a", True), ("b", True), ("c", False), max_blocks=max_blocks)[0] is None


# ---- 6. fused stats ----
def case_stats_exact(st, backend, size, dtype, two, nontemporal=False):
    r = Runner(st, backend, size, dtype)
    got, _, want = r.run(2, -3 if two else None, ("a", True), ("b", True), ("c", False), data="exact", stats=True,
                         nontemporal=nontemporal)
    rc.check_exact(got, rc.expect_exact(want.to(torch.int64)), f"{size} {dtype} two={two}")
    assert rc.fields(got) == rc.fields(field_reduce(r.dd, 0, r.q["a"]))


def case_stats_random(st, backend, dtype):
    """each sum within 2 n 2^-53 sum |t_i| of math.fsum of the oracle's terms (reduce_cases.case_random's bound: the
    any-order summation bound gamma_n sum |t_i|); min / max exact"""
    r = Runner(st, backend, RANDOM_SIZE, dtype)
    got, _, want = r.run(1, -0.7, ("a", True), ("a", True), ("b", False), stats=True)
    v = want.numpy().astype(np.float64).ravel()
    n = v.size
    assert got.count == n and got.nonfinite == 0 and got.dot == 0, rc.fields(got)
    for k, t in {"sum": v, "sum_abs": np.abs(v), "sum_sq": v * v}.items():
        ref, mag = math.fsum(t), math.fsum(np.abs(t))
        err, bound = abs(getattr(got, k) - ref), 2 * n * 2.0 ** -53 * mag
        print(f"{k}: got {getattr(got, k)!r} ref {ref!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{k}: |{getattr(got, k)!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
    assert got.min == v.min() and got.max == v.max(), (rc.fields(got), v.min(), v.max())


def case_stats_nonfinite(st, backend, dtype):
    """a NaN and an Inf planted in x are counted and land in dst"""
    planted = {(5, 3, 2): math.nan, (36, 10, 8): math.inf}
    r = Runner(st, backend, (37, 11, 9), dtype)
    got, _, want = r.run(0.5, 1, ("a", True), ("b", True), ("c", True), planted=planted, stats=True)
    assert got.count == want.numel() and got.nonfinite == 2 and math.isnan(got.sum), rc.fields(got)
    assert got.max == math.inf and math.isfinite(got.min), rc.fields(got)
    dst = get(r.dd, r.q["a"], True, dtype)
    assert math.isnan(dst[2, 3, 5]) and dst[8, 10, 36] == math.inf
    # a zero coefficient is multiplied like any other: 0 * NaN and 0 * Inf are NaN
    got, _, _ = r.run(0, 1, ("a", True), ("b", True), ("c", True), planted=planted, stats=True)
    assert got.nonfinite == 2 and got.max < math.inf, rc.fields(got)
    dst = get(r.dd, r.q["a"], True, dtype)
    assert math.isnan(dst[2, 3, 5]) and math.isnan(dst[8, 10, 36])


def case_stats_repeatable(st, backend, dtype):
    r = Runner(st, backend, RANDOM_SIZE, dtype)
    outs = [rc.bits(r.run(1.3, 2.9, ("a", True), ("b", True), ("c", False), stats=True)[0]) for _ in range(5)]
    assert all(o == outs[0] for o in outs), [o.hex() for o in outs]


# ---- 8. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    dd, qa, qb, (qi, qd) = make_domain(st, backend, size, torch.float32, extra=(torch.int32, torch.float64))
    for fn in (field_axpby, field_axpby_launch_info):
        for args in ((qi, 1.0, qa), (qa, 1.0, qi), (qa, 1.0, qb, 1.0, qi)):
            with pytest.raises(Exception, match="fp32 / fp64"):
                fn(dd, 0, *args)
        for args in ((qd, 1.0, qa), (qa, 1.0, qd), (qa, 1.0, qb, 1.0, qd)):
            with pytest.raises(Exception, match="differ in type"):
                fn(dd, 0, *args)
        for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
            with pytest.raises(Exception, match="outside compute region"):
                fn(dd, 0, qa, 1.0, qb, region=rect(lo, hi))
        for mb in (-1, (1 << 20) + 1):
            with pytest.raises(Exception, match="maxBlocks"):
                fn(dd, 0, qa, 1.0, qb, max_blocks=mb)
        for di in (1, 7):
            with pytest.raises(Exception):
                fn(dd, di, qa, 1.0, qb)
        fn(dd, 0, qa, 1.0, qb, max_blocks=1 << 20, region=rect((4, 4, 4), (4, 9, 7)))  # the bound itself is taken
    assert not field_axpby_supported(dd, 0, qi, qa) and not field_axpby_supported(dd, 0, qa, qb, qd)
    assert field_axpby_supported(dd, 0, qa, qb) and field_axpby_supported(dd, 0, qd, qd, qd)
    # an unrealized domain has no sub-domain to take
    und = st.DistributedDomain(*size, group=st.make_single_group())
    und.set_backend(backend)
    q0 = und.add_data("a", torch.float32)
    for fn in (field_axpby, field_axpby_launch_info):
        with pytest.raises(Exception):
            fn(und, 0, q0, 1.0, q0, region=rect((0, 0, 0), (1, 1, 1)))
    with pytest.raises(Exception, match="realize"):
        und.axpby(q0, 1.0, q0)
    # the refusals of dd.axpby come before anything is written
    for q in (qa, qb):
        dd.domain(0).fill_bytes(q, FILL, True, True)
    before = dd.domain(0).buffer_to_host(qa, True)
    with pytest.raises(Exception, match="differ in type"):
        dd.axpby(qa, 1.0, qb, 1.0, qd)
    rc.sync(dd)
    assert dd.domain(0).buffer_to_host(qa, True) == before


# ---- 9. several sub-domains ----
def case_dd(st, backend, gpus):
    dtype = torch.float32
    dd, qa, qb, (qc,) = make_domain(st, backend, DD_SIZE, dtype, gpus=gpus, extra=(dtype,))
    assert dd.num_domains() == len(gpus)
    rc.poison(dd, [qa, qb, qc])
    X, Y = random_field(DD_SIZE, dtype, 61), random_field(DD_SIZE, dtype, 62)
    put(dd, qb, True, X)
    put(dd, qc, False, Y)
    assert dd.axpby(qa, 1.3, qb, 2.9, qc, y_curr=False) is None
    assert same_bits(get(dd, qa, True, dtype), axpby_reference(1.3, X, 2.9, Y))
    dd.copy(qa, qc, dst_curr=False, src_curr=False)
    assert same_bits(get(dd, qa, False, dtype), Y)
    dd.scale(qa, 0.375, curr=False)
    assert same_bits(get(dd, qa, False, dtype), axpby_reference(0.375, Y))
    assert same_bits(get(dd, qc, False, dtype), Y) and same_bits(get(dd, qb, True, dtype), X)
    # stats on integer data: exact, collective or local (one rank)
    A, B = exact_field(DD_SIZE, 21), exact_field(DD_SIZE, 22)
    put(dd, qb, True, A.to(dtype))
    put(dd, qc, True, B.to(dtype))
    want = rc.expect_exact(2 * A - 3 * B)
    s = dd.axpby(qa, 2, qb, -3, qc, stats=True)
    rc.check_exact(s, want, "dd.axpby stats")
    loc = dd.axpby(qa, 2, qb, -3, qc, stats=True, local=True)
    assert rc.bits(loc) == rc.bits(s)
    assert rc.fields(dd.reduce(qa)) == rc.fields(s)
    assert same_bits(get(dd, qa, True, dtype), (2 * A - 3 * B).to(dtype))


# ---- 11. StarCG against a torch CG ----
def helmholtz():
    return star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])  # I - Laplacian


def poisson():
    return star_weights(1, 6.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])


def walls(z_value=0.0):
    """x periodic, y mirror, z antimirror(z_value)"""
    FC = _C.FaceCondition
    bc = _C.BoundaryConditions()
    bc.set_axis(1, FC.mirror(), FC.mirror())
    bc.set_axis(2, FC.antimirror(z_value), FC.antimirror(z_value))
    return bc


CG_SIZE = (16, 12, 10)
CG_CASES = {
    "helmholtz_periodic": (helmholtz, None),
    "helmholtz_walls": (helmholtz, 0.0),
    "poisson_walls": (poisson, 0.0),
    "poisson_walls_0.25": (poisson, 0.25),
    "poisson_walls_1.0": (poisson, 1.0),
}
CG_TOL = {torch.float64: 1e-10, torch.float32: 1e-4}


def homogeneous(bc):
    from stencil2_amd.models.star_cg import _conditions
    return None if bc is None else _conditions(bc, True)


def oracle_cg(w, bc, f, tol, max_iters):
    """the algorithm of StarCG.solve on the global grid: fields in f's dtype through axpby_reference, A through
    star_step_reference (pad_reference under the conditions), reductions in float64"""
    def ssq(v):
        return float((v.double() * v.double()).sum())

    hom = homogeneous(bc)
    u = torch.zeros_like(f)
    ff = ssq(f)
    r = axpby_reference(1.0, f, -1.0, star_step_reference(u, w, boundary=bc))
    rr = ssq(r)
    p = r.clone()
    it = 0
    while it < max_iters and math.sqrt(rr / ff) >= tol:
        Ap = star_step_reference(p, w, boundary=hom)
        alpha = rr / float((p.double() * Ap.double()).sum())
        u = axpby_reference(1.0, u, alpha, p)
        r = axpby_reference(1.0, r, -alpha, Ap)
        rr_new = ssq(r)
        p = axpby_reference(1.0, r, rr_new / rr, p)
        rr = rr_new
        it += 1
    return it, math.sqrt(rr / ff), u


@functools.lru_cache(maxsize=None)
def cg_oracle(name, dtype):
    """(iters, relres) of the oracle for a case (computed once, shared)"""
    wf, zv = CG_CASES[name]
    it, rel, _ = oracle_cg(wf(), None if zv is None else walls(zv), cg_rhs(dtype), CG_TOL[dtype], 1000)
    return it, rel


def cg_rhs(dtype):
    return random_field(CG_SIZE, dtype, 51)


def gather_solution(m):
    dd = m.domain
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=m.dtype)
    m.synchronize()
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.solution(di).cpu()
    return out


def make_cg(st, backend, w, bc, dtype, gpus=(0,), f=None, group=None, methods=None, size=CG_SIZE):
    kw = {} if methods is None else dict(methods=methods)
    m = st.StarCG(size, w, fp64=dtype == torch.float64, gpus=list(gpus), backend=backend, boundary=bc,
                  group=group if group is not None else st.make_single_group(), **kw)
    f = cg_rhs(dtype) if f is None else f
    X, Y, Z = size
    m.set_rhs(lambda gz, gy, gx: f.to(gz.device)[gz % Z, gy % Y, gx % X])
    return m, f


def true_residual(u, f, w, bc):
    """||f - A u||2 / ||f||2 in float64 torch (A under `bc`, inhomogeneous values included)"""
    r = f.double() - star_step_reference(u.double(), w, boundary=bc)
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


def case_cg(st, backend, name, dtype, gpus=(0,)):
    wf, zv = CG_CASES[name]
    w, bc, tol = wf(), None if zv is None else walls(zv), CG_TOL[dtype]
    m, f = make_cg(st, backend, w, bc, dtype, gpus)
    assert m.domain.num_domains() == len(gpus)
    iters, relres = m.solve(tol=tol, max_iters=1000)
    want_iters, want_rel = cg_oracle(name, dtype)
    true = true_residual(gather_solution(m), f, w, bc)
    print(f"{name} {dtype}: iters {iters} relres {relres:.3e} true {true:.3e}; oracle iters {want_iters} relres {want_rel:.3e}")
    assert relres < tol and true <= 2 * tol, (relres, true, tol)
    assert abs(iters - want_iters) <= 1, (iters, want_iters)
    return m


def case_cg_limits(st, backend):
    """max_iters, a NaN in f, f = 0, asymmetric weights and an Open wall"""
    dtype, name = torch.float64, "helmholtz_walls"
    w, bc = helmholtz(), walls(0.0)
    want_iters, _ = cg_oracle(name, dtype)
    m, f = make_cg(st, backend, w, bc, dtype)
    it, rel = m.solve(tol=CG_TOL[dtype], max_iters=0)
    assert (it, rel) == (0, 1.0) and not gather_solution(m).any()  # u0 = 0: r0 = f
    cap = want_iters // 2
    m, _ = make_cg(st, backend, w, bc, dtype)
    it, rel = m.solve(tol=CG_TOL[dtype], max_iters=cap)
    assert it == cap and CG_TOL[dtype] <= rel < 1.0, (it, rel, cap)
    # continuing from the capped u reaches the tolerance (the guess is the current u)
    it2, rel2 = m.solve(tol=CG_TOL[dtype], max_iters=1000)
    assert rel2 < CG_TOL[dtype] and true_residual(gather_solution(m), f, w, bc) <= 2 * CG_TOL[dtype]
    bad = f.clone()
    bad[3, 4, 5] = math.nan
    m, _ = make_cg(st, backend, w, bc, dtype, f=bad)
    with pytest.raises(FloatingPointError):
        m.solve()
    m, _ = make_cg(st, backend, w, bc, dtype, f=torch.zeros_like(f))
    m.set_guess(lambda gz, gy, gx: (gz + gy + gx).to(torch.float64))
    assert m.solve() == (0, 0.0) and not gather_solution(m).any()
    with pytest.raises(ValueError, match="symmetric"):
        st.StarCG(CG_SIZE, star_weights(1, 7.0, [-1.0, -1.5], [-1.0, -1.0], [-1.0, -1.0]), backend=backend, gpus=[0],
                  group=st.make_single_group())
    op = _C.BoundaryConditions()
    op.set_axis(2, _C.FaceCondition.open(), _C.FaceCondition.mirror())
    with pytest.raises(ValueError, match="Open"):
        st.StarCG(CG_SIZE, w, backend=backend, gpus=[0], group=st.make_single_group(), boundary=op)


# ---- 12. second-order accuracy of the walls ----
def case_wall_order(st, backend):
    """-u'' = (pi / L)^2 sin(pi x / L) between antimirror(0) x walls, cell-centred, L = 1: the max error against
    sin(pi x / L) falls by 4 (second order; a factor in [3.5, 4.5]) from 16 to 32 cells"""
    FC = _C.FaceCondition
    errs = []
    for n in (16, 32):
        h = 1.0 / n
        w = star_weights(1, 6.0 / h ** 2, [-1.0 / h ** 2] * 2, [-1.0 / h ** 2] * 2, [-1.0 / h ** 2] * 2)
        bc = _C.BoundaryConditions()
        bc.set_axis(0, FC.antimirror(0.0), FC.antimirror(0.0))
        m = st.StarCG((n, 4, 4), w, fp64=True, gpus=[0], backend=backend, boundary=bc, group=st.make_single_group())
        m.set_rhs(lambda gz, gy, gx: math.pi ** 2 * torch.sin(math.pi * (gx.double() + 0.5) * h) + 0 * (gy + gz))
        iters, relres = m.solve(tol=1e-12, max_iters=200)
        assert relres < 1e-12, (iters, relres)
        x = (torch.arange(n, dtype=torch.float64) + 0.5) * h
        errs.append(float((gather_solution(m) - torch.sin(math.pi * x).view(1, 1, -1)).abs().max()))
    ratio = errs[0] / errs[1]
    print(f"wall order: errors {errs}, ratio {ratio:.4f}")
    assert 3.5 <= ratio <= 4.5, (errs, ratio)


def hexline(s):
    return " ".join(f"{k}={float(getattr(s, k)).hex()}" for k in rc.FIELDS)
