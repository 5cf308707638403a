"""Cases shared by test_reduce.py (host backend, the plain loop) and test_gpu_reduce.py (the HIP kernels of
csrc/src/kernels/field_reduce.hip): FieldStats of one operand, or of the difference and dot product of two.

Unless a case says otherwise every byte of both buffers of every quantity is first set to 0xFF (a NaN in fp32 and
fp64), then only the cells to be reduced are written: a halo, padding or out-of-region cell that leaks into the
result shows as NaN, as a non-zero `nonfinite` or as a wrong exact value.

Exact data are seeded integers in [-7, 7]: every partial sum of e, |e|, e * e and a * b stays far below 2^53, so any
summation order gives exactly the int64 torch values. Random data are compared within the any-order summation bound
gamma_n * sum |t_i| (see case_random)."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import field_reduce, field_reduce_launch_info, field_reduce_supported

FIELDS = ("count", "nonfinite", "sum", "sum_abs", "sum_sq", "min", "max", "dot")

SIZES = [(1, 1, 1), (3, 2, 2), (5, 1, 7), (37, 11, 9), (256, 2, 3), (257, 3, 2), (260, 5, 1), (513, 1, 1), (131, 17, 33)]
SIZES_F64 = [(128, 2, 3), (129, 3, 2)]
DTYPES = [torch.float32, torch.float64]
# (operand a is curr?, operand b is curr?): a on curr and b on next, and swapped
OPERANDS = [(True, False), (False, True)]
SHAPE_CASES = [(s, dt) for dt in DTYPES for s in SIZES] + [(s, torch.float64) for s in SIZES_F64]
FORCED = [(size, mb) for size in ((37, 11, 9), (257, 3, 2)) for mb in (1, 2, 7, 1000)]
RANDOM_SIZE = (131, 17, 33)
DD_SIZE = (40, 24, 36)


def dtype_id(dt):
    return str(dt).split(".")[-1]


def shape_id(case):
    return "x".join(map(str, case[0])) + "-" + dtype_id(case[1])


def sub_regions(size):
    """star_cases.sub_regions plus the whole region: off-chunk x start and end, single cell / row / plane, empty"""
    from star_cases import sub_regions as star_regions
    r = dict(star_regions(size))
    r["whole"] = ((0, 0, 0), tuple(size))
    r["one_row"] = ((0, 6, 4), (size[0], 7, 5))
    return r


@functools.lru_cache(maxsize=None)
def exact_field(size, seed):
    """seeded integers in [-7, 7] as an int64 (z, y, x) tensor (shared, never modified)"""
    X, Y, Z = size
    return torch.randint(-7, 8, (Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def random_field(size, dtype, seed):
    """seeded uniform [-1, 1) (z, y, x) tensor of dtype"""
    X, Y, Z = size
    return torch.rand((Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=dtype) * 2 - 1


def make_domain(st, backend, size, dtype, gpus=(0,), radius=1, group=None, methods=None, opaque=0, extra=(), **layout):
    """two quantities a, b of `dtype` (opaque: of that many opaque bytes) plus `extra` dtypes; layout: interior_align,
    shared_halo_line, padding, x_halo_align"""
    dd = st.DistributedDomain(*size, group=group if group is not None else st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius if not isinstance(radius, int) else st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus(list(gpus))
    if methods is not None:
        dd.set_methods(methods)
    if "interior_align" in layout:
        dd.set_interior_align(layout["interior_align"])
    if layout.get("shared_halo_line"):
        dd.set_shared_halo_line(True)
    if layout.get("padding") is False:
        dd.set_padding(False)
    if layout.get("x_halo_align"):
        dd.set_x_halo_align(True)
    if opaque:
        qa, qb = dd.native.add_data(opaque, "a"), dd.native.add_data(opaque, "b")
    else:
        qa, qb = dd.add_data("a", dtype), dd.add_data("b", dtype)
    qx = [dd.add_data(f"x{i}", dt) for i, dt in enumerate(extra)]
    dd.realize()
    return dd, qa, qb, qx


def sync(dd):
    if dd.backend() == _C.Backend.Device:
        torch.cuda.synchronize()


def poison(dd, qs):
    for di in range(dd.num_domains()):
        for q in qs:
            dd.domain(di).fill_bytes(q, 0xFF, True, True)
    sync(dd)


def put(dd, q, curr, u, lo=(0, 0, 0), hi=None):
    """write the cells [lo, hi) (global x, y, z) of the global (z, y, x) tensor u into quantity q (curr or next) of
    every sub-domain that holds some of them; nothing else is written"""
    X, Y, Z = u.shape[2], u.shape[1], u.shape[0]
    hi = (X, Y, Z) if hi is None else hi
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s, ao = d.origin(), d.size(), d.accessor_origin()
        l = (max(lo[0], o.x), max(lo[1], o.y), max(lo[2], o.z))
        h = (min(hi[0], o.x + s.x), min(hi[1], o.y + s.y), min(hi[2], o.z + s.z))
        if any(h[i] <= l[i] for i in range(3)):
            continue
        part = u[l[2]:h[2], l[1]:h[1], l[0]:h[0]].contiguous()
        d.region_from_host(_C.Dim3(l[0] - ao.x, l[1] - ao.y, l[2] - ao.z), _C.Dim3(h[0] - l[0], h[1] - l[1], h[2] - l[2]),
                           q, part.numpy().tobytes(), curr)
    sync(dd)


def rect(lo, hi):
    return _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))


def fields(s):
    return {k: getattr(s, k) for k in FIELDS}


def bits(s):
    """the struct's fields as bytes (doubles through struct.pack('d'))"""
    return b"".join(struct.pack("q", getattr(s, k)) if k in ("count", "nonfinite") else struct.pack("d", getattr(s, k))
                    for k in FIELDS)


def expect_exact(a, b=None):
    """the exact FieldStats of int64 tensors a (and b)"""
    e = a if b is None else a - b
    n = e.numel()
    return {"count": n, "nonfinite": 0, "sum": int(e.sum()), "sum_abs": int(e.abs().sum()), "sum_sq": int((e * e).sum()),
            "min": int(e.min()) if n else math.inf, "max": int(e.max()) if n else -math.inf,
            "dot": 0 if b is None else int((a * b).sum())}


def check_exact(got, want, what=""):
    g = fields(got)
    for k in FIELDS:
        assert g[k] == want[k], f"{what}: {k} = {g[k]!r}, want {want[k]!r} ({g})"


IDENTITY = {"count": 0, "nonfinite": 0, "sum": 0, "sum_abs": 0, "sum_sq": 0, "min": math.inf, "max": -math.inf, "dot": 0}


def expected_path(backend, device_path):
    return device_path if backend == _C.Backend.Device else "host"


# ---- 1. exact data over shapes, operands, forced grids, sub-regions and layouts ----
def case_exact(st, backend, size, dtype, two, a_curr=True, b_curr=False, lo=(0, 0, 0), hi=None, max_blocks=0,
               device_path="fast", opaque=0, same_quantity=False, **layout):
    """operand a = (qa, a_curr), operand b = (qb, b_curr) (same_quantity: qb = qa, the two buffers of one quantity);
    only the cells of [lo, hi) are written, everything else stays NaN"""
    hi = tuple(size) if hi is None else hi
    dd, qa, qb, _ = make_domain(st, backend, size, dtype, opaque=opaque, **layout)
    if same_quantity:
        assert two and a_curr != b_curr
        qb = qa
    poison(dd, [qa, qb])
    A, B = exact_field(tuple(size), 21), exact_field(tuple(size), 22)
    put(dd, qa, a_curr, A.to(dtype), lo, hi)
    if two:
        put(dd, qb, b_curr, B.to(dtype), lo, hi)
    region = rect(lo, hi)
    kw = dict(other=qb if two else None, curr=a_curr, other_curr=b_curr, region=region, max_blocks=max_blocks)
    info = field_reduce_launch_info(dd, 0, qa, **kw)
    empty = any(hi[i] <= lo[i] for i in range(3))
    assert info["path"] == ("none" if empty else expected_path(backend, device_path)), info
    if not empty:
        ny, nz = hi[1] - lo[1], hi[2] - lo[2]
        assert info["items"] == ny * nz, info
        if backend == _C.Backend.Device:
            if max_blocks:
                assert info["blocks"] == max_blocks, info
            else:
                assert 1 <= info["blocks"] <= ny * nz, info
    assert field_reduce_supported(dd, 0, qa, qb if two else None)
    got = field_reduce(dd, 0, qa, stream=0, **kw)
    sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    want = IDENTITY if empty else expect_exact(A[sl], B[sl] if two else None)
    check_exact(got, want, f"{size} {dtype} two={two} [{lo}, {hi}) blocks {max_blocks} {info}")
    if empty:
        assert got.linf == 0.0 and got.l1 == 0.0 and got.l2 == 0.0
    else:
        assert got.l1 == want["sum_abs"] and got.l2 == math.sqrt(want["sum_sq"])
        assert got.linf == max(-want["min"], want["max"])
    return got, info


def case_forced_grid(st, backend, size, dtype, two, max_blocks):
    """a forced grid gives the same exact result as the automatic one (1000 blocks leave blocks with no work)"""
    auto, _ = case_exact(st, backend, size, dtype, two)
    forced, info = case_exact(st, backend, size, dtype, two, max_blocks=max_blocks)
    assert fields(auto) == fields(forced), (fields(auto), fields(forced), info)


def asymmetric_radius(st):
    """face radius 3 on -x only, 0 everywhere else"""
    r = st.Radius.face_edge_corner(0, 0, 0)
    r.set_dir(-1, 0, 0, 3)
    return r


# name -> (layout keywords, the device path)
LAYOUTS = {
    "align64": (dict(interior_align=64), "fast"),
    "align128": (dict(interior_align=128), "fast"),
    "shared_halo_line": (dict(shared_halo_line=True), "fast"),
    "asymmetric_radius": (dict(radius="asym"), "fast"),
    "unpadded": (dict(padding=False), "generic"),
    "x_halo_align": (dict(x_halo_align=True), "generic"),
}


def case_layout(st, backend, name, dtype, two):
    kw, path = LAYOUTS[name]
    kw = dict(kw)
    if kw.get("radius") == "asym":
        kw["radius"] = asymmetric_radius(st)
    got, info = case_exact(st, backend, (37, 11, 9), dtype, two, device_path=path, **kw)
    return info


def case_opaque(st, backend, es, two):
    """opaque 4- / 8-byte elements are taken as fp32 / fp64"""
    case_exact(st, backend, (37, 11, 9), torch.float32 if es == 4 else torch.float64, two, opaque=es)


# ---- 2. non-finite cells ----
def case_nonfinite(st, backend, dtype, two, only_nan):
    size = (37, 11, 9)
    dd, qa, qb, _ = make_domain(st, backend, size, dtype)
    poison(dd, [qa, qb])
    A, B = exact_field(size, 21).to(dtype).clone(), exact_field(size, 22).to(dtype)
    planted = {(5, 3, 2): math.nan} if only_nan else {(5, 3, 2): math.nan, (36, 10, 8): math.inf, (0, 0, 4): -math.inf}
    for (x, y, z), v in planted.items():
        A[z, y, x] = v
    put(dd, qa, True, A)
    if two:
        put(dd, qb, False, B)
    got = field_reduce(dd, 0, qa, other=qb if two else None, curr=True, other_curr=False)
    e = A.double() - B.double() if two else A.double()
    assert got.count == e.numel() and got.nonfinite == len(planted), fields(got)
    assert math.isnan(got.sum) and math.isnan(got.linf), fields(got)
    keep = ~torch.isnan(e)
    if only_nan:
        assert got.min == float(e[keep].min()) and got.max == float(e[keep].max()), fields(got)
        assert math.isfinite(got.min) and math.isfinite(got.max)
    else:
        assert got.min == -math.inf and got.max == math.inf, fields(got)


# ---- 3. random data within the any-order summation bound ----
@functools.lru_cache(maxsize=None)
def random_terms(dtype, two):
    """float64 numpy terms t_i of sum, sum_abs, sum_sq and dot of the random case, and min / max of e"""
    a = random_field(RANDOM_SIZE, dtype, 31).numpy().astype(np.float64).ravel()
    b = random_field(RANDOM_SIZE, dtype, 32).numpy().astype(np.float64).ravel()
    e = a - b if two else a
    return {"sum": e, "sum_abs": np.abs(e), "sum_sq": e * e, "dot": a * b if two else np.zeros_like(a)}, e.min(), e.max()


def random_domain(st, backend, dtype, two):
    dd, qa, qb, _ = make_domain(st, backend, RANDOM_SIZE, dtype)
    poison(dd, [qa, qb])
    put(dd, qa, True, random_field(RANDOM_SIZE, dtype, 31))
    if two:
        put(dd, qb, False, random_field(RANDOM_SIZE, dtype, 32))
    return dd, qa, qb


def case_random(st, backend, dtype, two):
    """|got - fsum(t)| <= 2 n 2^-53 fsum(|t|): the any-order summation bound gamma_n sum |t_i|, the factor 2 covering
    the rounding of each term and the higher-order remainder at n <= 2^20; min / max exact"""
    dd, qa, qb = random_domain(st, backend, dtype, two)
    got = field_reduce(dd, 0, qa, other=qb if two else None, curr=True, other_curr=False)
    terms, emin, emax = random_terms(dtype, two)
    n = terms["sum"].size
    assert got.count == n and got.nonfinite == 0, fields(got)
    for k, t in terms.items():
        ref, mag = math.fsum(t), math.fsum(np.abs(t))
        err, bound = abs(getattr(got, k) - ref), 2 * n * 2.0 ** -53 * mag
        print(f"{k}: got {getattr(got, k)!r} ref {ref!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{k}: |{getattr(got, k)!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
    assert got.min == emin and got.max == emax, (fields(got), emin, emax)
    if not two:
        assert got.dot == 0


def case_repeatable(st, backend, dtype):
    """the random two-operand case five times: bitwise identical structs"""
    dd, qa, qb = random_domain(st, backend, dtype, True)
    outs = [bits(field_reduce(dd, 0, qa, other=qb, curr=True, other_curr=False)) for _ in range(5)]
    assert all(o == outs[0] for o in outs), [o.hex() for o in outs]


# ---- 4. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    dd, qa, qb, (qi, qd) = make_domain(st, backend, size, torch.float32, extra=(torch.int32, torch.float64))
    for fn in (field_reduce, field_reduce_launch_info):
        with pytest.raises(Exception, match="fp32 / fp64"):
            fn(dd, 0, qi)
        with pytest.raises(Exception, match="fp32 / fp64"):
            fn(dd, 0, qa, other=qi)
        with pytest.raises(Exception, match="differ in type"):
            fn(dd, 0, qa, other=qd)
        for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
            with pytest.raises(Exception, match="outside compute region"):
                fn(dd, 0, qa, region=rect(lo, hi))
        for di in (1, 7):
            with pytest.raises(Exception):
                fn(dd, di, qa)
    assert not field_reduce_supported(dd, 0, qi) and not field_reduce_supported(dd, 0, qa, qd)
    assert field_reduce_supported(dd, 0, qa, qb) and field_reduce_supported(dd, 0, qd)
    with pytest.raises(ValueError):
        dd.norm(qa, p=3)


# ---- 5. several sub-domains: DistributedDomain.reduce, norm, dot, residual ----
def fill_dd(dd, qa, qb, A, B):
    """curr(qa) = A, next(qa) = B, curr(qb) = B over a poisoned allocation"""
    poison(dd, [qa, qb])
    put(dd, qa, True, A)
    put(dd, qa, False, B)
    put(dd, qb, True, B)


def case_dd_exact(st, backend, gpus):
    """dd.reduce over several sub-domains equals the exact values (and so the one-sub-domain result)"""
    A, B = exact_field(DD_SIZE, 21), exact_field(DD_SIZE, 22)
    dd, qa, qb, _ = make_domain(st, backend, DD_SIZE, torch.float32, gpus=gpus)
    assert dd.num_domains() == len(gpus)
    fill_dd(dd, qa, qb, A.float(), B.float())
    one = dd.reduce(qa)
    check_exact(one, expect_exact(A), "reduce(qa)")
    check_exact(dd.reduce(qa, curr=False), expect_exact(B), "reduce(qa, curr=False)")
    res = dd.residual(qa)
    check_exact(res, expect_exact(A, B), "residual(qa)")
    check_exact(dd.reduce(qa, other=qb, other_curr=True), expect_exact(A, B), "reduce(qa, other=qb)")
    check_exact(dd.reduce(qa, local=True), expect_exact(A), "reduce(qa, local=True)")
    assert dd.norm(qa, 1) == one.l1 and dd.norm(qa) == one.l2 and dd.norm(qa, "inf") == one.linf
    assert dd.norm(qa, 2) == math.sqrt(int((A * A).sum()))
    assert dd.dot(qa, qb) == int((A * B).sum()) == dd.reduce(qa, other=qb, other_curr=True).dot
    assert fields(res) == fields(dd.reduce(qa, other=qa, other_curr=False))


# ---- 6. run_until against the torch oracles ----
def oracle_checks(step, u, check_every, checks):
    """max |u_new - u_old| (float64, exact) of the last step of every block of check_every steps"""
    vals = []
    for _ in range(checks):
        for _ in range(check_every):
            old, u = u, step(u)
        vals.append(float((u.double() - old.double()).abs().max()))
    return vals


def pick_tol(vals):
    """a tolerance the oracle first meets at check 3..6 (1-based): halfway below everything seen before"""
    for k in range(2, 6):
        if vals[k] < min(vals[:k]):
            return 0.5 * (vals[k] + min(vals[:k])), k + 1
    raise AssertionError(f"no check 3..6 improves on the ones before: {vals}")


def gather_model(m):
    dd = m.domain
    out = None
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        t = m.interior(di).cpu()
        if out is None:
            g = dd.size()
            out = torch.empty((g.z, g.y, g.x), dtype=t.dtype)
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = t
    return out


def case_run_until_star(st, backend, gpus=(0,)):
    from stencil2_amd.ops import diffusion_star, star_step_reference
    size, w, every = (16, 16, 16), diffusion_star(2, 0.1), 4
    u0 = torch.rand((16, 16, 16), generator=torch.Generator().manual_seed(41))
    vals = oracle_checks(lambda u: star_step_reference(u, w), u0, every, 8)
    tol, k = pick_tol(vals)

    def model():
        m = st.StarStencil3D(size, w, gpus=list(gpus), backend=backend)
        m.init(lambda gz, gy, gx: u0.to(gz.device)[gz % 16, gy % 16, gx % 16])
        return m
    m = model()
    done, value = m.run_until(tol, 1000, check_every=every, norm="inf")
    assert (done, value) == (every * k, vals[k - 1]), (done, value, k, vals)
    u = u0
    for _ in range(done):
        u = star_step_reference(u, w)
    assert torch.equal(gather_model(m), u)
    # max_iters is honoured when nothing can be below tol = 0 (the last block is shorter)
    m = model()
    done, value = m.run_until(0.0, 10, check_every=every)
    u, old = u0, None
    for _ in range(10):
        old, u = u, star_step_reference(u, w)
    assert (done, value) == (10, float((u.double() - old.double()).abs().max()))
    assert m.run_until(0.0, 0) == (0, math.inf)
    # the other norms are those of dd.residual
    r = m.domain.residual(0)
    m2 = model()
    m2.run(9)
    assert m2.run_until(0.0, 1, norm=2) == (1, r.l2) and r.l2 > 0
    for bad in (dict(check_every=0), dict(norm="max"), dict(max_iters=-1)):
        with pytest.raises(ValueError):
            m.run_until(**{**dict(tol=1.0, max_iters=4), **bad})
    # a NaN in the field raises at the first check
    m = model()
    m.interior(0)[3, 4, 5] = math.nan
    with pytest.raises(FloatingPointError):
        m.run_until(1e-3, 100, check_every=every)


@functools.lru_cache(maxsize=None)
def jacobi_oracle(every):
    """the seeded (32, 32, 32) start field and the oracle's value at each of 8 checks (computed once, shared)"""
    from stencil2_amd.ops import jacobi_step_reference
    u0 = torch.rand((32, 32, 32), generator=torch.Generator().manual_seed(42))
    return u0, oracle_checks(jacobi_step_reference, u0, every, 8)


def case_run_until_jacobi(st, backend, temporal=1, **kw):
    """temporal > 1: run(check_every - 1) advances in fused pairs / triples where the kernels take the shape, and the
    block's last step is always a single step()"""
    from stencil2_amd.ops import jacobi_step_reference
    size, every = (32, 32, 32), 4
    u0, vals = jacobi_oracle(every)
    tol, k = pick_tol(vals)

    def model():
        m = st.Jacobi3D(size, gpus=[0], backend=backend, temporal=temporal, **kw)
        m.init()
        assert m.forwarding() == bool(kw.get("forward"))
        m.interior(0).copy_(u0)
        m.synchronize()
        sync(m.domain)
        m.domain.exchange()  # the new field's halos (a forwarding model never exchanges again)
        return m
    m = model()
    done, value = m.run_until(tol, 1000, check_every=every, norm="inf")
    assert (done, value) == (every * k, vals[k - 1]), (done, value, k, vals)
    u = u0
    for _ in range(done):
        u = jacobi_step_reference(u)
    assert torch.equal(m.interior(0).cpu(), u)
    m = model()
    assert m.run_until(0.0, 6, check_every=every)[0] == 6
    m = model()
    m.interior(0)[3, 4, 5] = math.nan
    sync(m.domain)
    with pytest.raises(FloatingPointError):
        m.run_until(1e-3, 100, check_every=every)
