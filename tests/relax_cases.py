"""Cases shared by test_relax.py (host backend, the plain loop) and test_gpu_relax.py (the HIP kernels of
csrc/src/kernels/stencil_varcoef_relax.hip): the fused residual / damped-Jacobi sweep of the variable-coefficient
operator, every comparison bitwise (`same_bits`, so NaN and inf patterns compare) against
stencil2_amd.ops.varcoef_relax_reference (torch on the CPU, one op per rounding).

u and f are torch.rand from two seeds, kappa is 0.5 + torch.rand from a third. Residual cases take the four random-sign
weights of varcoef_cases.random_weights; Jacobi cases a seeded shift in (0, 1) and three distinct negative h, so the
diagonal shift - sum h (kappa(c) + kappa(n)) is >= shift > 0 and no quotient is NaN. omega = 6 / 7."""
import functools

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (axpby_reference, varcoef_relax, varcoef_relax_launch_info, varcoef_relax_reference,
                              varcoef_relax_supported, varcoef_step_reference, varcoef_weights)

from algebra_cases import same_bits
from star_cases import MODEL_CASES, SENTINEL, SHAPES, dtype_id, sub_regions  # noqa: F401  (shared shapes)
from stencil7_cases import FILL
from varcoef_cases import global_kappa, global_u, mirror_twin, random_weights, wall_conditions

DTYPES = [torch.float32, torch.float64]
MODES = ["residual", "jacobi"]
F_SEED, V_SEED, JW_SEED = 41, 67, 733
OMEGA = 6.0 / 7.0


def jacobi_weights(seed=JW_SEED):
    """shift in (0, 1) and hx, hy, hz: three distinct values in (-1, 0)"""
    v = torch.rand(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).tolist()
    assert len(set(v)) == 4 and all(0 < a < 1 for a in v)
    return varcoef_weights(v[0], -v[1], -v[2], -v[3])


def mode_weights(mode):
    return random_weights() if mode == "residual" else jacobi_weights()


def mode_omega(mode):
    return None if mode == "residual" else OMEGA


def global_f(size, dtype):
    return global_u(size, dtype, seed=F_SEED)


@functools.lru_cache(maxsize=None)
def oracle(size, dtype, mode, sweeps=1, walls=None):
    """`sweeps` reference sweeps (each from the one before; the residual: one) of the case's fields (computed once)"""
    u, k, f, w = global_u(size, dtype), global_kappa(size, dtype), global_f(size, dtype), mode_weights(mode)
    bc, kbc = wall_conditions(walls)
    if bc is not None and kbc is None:
        kbc = mirror_twin(bc)
    for _ in range(sweeps):
        u = varcoef_relax_reference(u, k, f, w, omega=mode_omega(mode), boundary=bc, kappa_boundary=kbc)
    return u


def make_domain(st, backend, size, dtype, radius=1, padding=True, dtypes=None):
    """one sub-domain with the quantities u, kappa, f and v (`dtypes`: their four dtypes, default all `dtype`)"""
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius if not isinstance(radius, int) else st.Radius.face_edge_corner(radius, 0, 0))
    dd.set_gpus([0])
    if not padding:
        dd.set_padding(False)
    qs = [dd.add_data(n, dt) for n, dt in zip(("u", "kappa", "f", "v"), dtypes or [dtype] * 4)]
    dd.realize()
    return (dd, *qs)


def _sync(dd):
    if dd.backend() == _C.Backend.Device:
        torch.cuda.synchronize()


def set_fields(dd, qs, size, dtype, kappa=None, f=None):
    """u, kappa and f of the case into the interiors of their curr buffers (one sub-domain), then the exchange"""
    qu, qk, qf = qs
    for q, g in ((qu, global_u(size, dtype)), (qk, global_kappa(size, dtype) if kappa is None else kappa),
                 (qf, global_f(size, dtype) if f is None else f)):
        t = dd.curr_interior(0, q)
        t.copy_(g.to(t.device))
    _sync(dd)
    dd.exchange()


def _tune(st, zchunk=0, alt=True):
    t = st.StencilTune()
    t.zchunk = zchunk
    t.alternate_z = alt
    return t


def _report(got, want, what):
    bad = int((got != want).sum())
    return f"{what}: {bad} of {want.numel()} cells differ, max {(got - want).abs().max().item()}"


# ---- 1. the kernel over shapes, both modes, both march directions, both buffer parities ----
def case_shape(st, backend, size, zchunk, dtype, mode, expect_fast=None):
    dd, qu, qk, qf, _ = make_domain(st, backend, size, dtype)
    w, om, want = mode_weights(mode), mode_omega(mode), oracle(size, dtype, mode)
    for parity in (0, 1):
        assert dd.domain(0).parity() == parity
        set_fields(dd, (qu, qk, qf), size, dtype)
        for alt in (True, False):
            tune = _tune(st, zchunk, alt)
            info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om, tune=tune)
            if expect_fast is not None:
                assert (info["path"] == "fast") == expect_fast, info
                if zchunk:
                    assert info["zchunk"] == zchunk and info["zchunks"] == -(-size[2] // zchunk), info
            else:
                assert info["path"] == "host", info
            dd.next(0, qu).fill_(SENTINEL)
            _sync(dd)
            varcoef_relax(dd, 0, qu, qk, qf, w, omega=om, tune=tune)
            _sync(dd)
            got = dd.interior(dd.next(0, qu), 0).cpu()
            assert same_bits(got, want), _report(got, want, f"{mode} parity {parity} alternate_z {alt} ({info})")
        dd.swap()


def case_tune_flags(st, backend, dtype, expect_fast=None):
    """non-temporal stores and the XCD-aware block order change no bit (two or three wave columns, three row groups, four z chunks)"""
    size = (257, 33, 17)
    dd, qu, qk, qf, _ = make_domain(st, backend, size, dtype)
    set_fields(dd, (qu, qk, qf), size, dtype)
    for mode in MODES:
        w, om, want = mode_weights(mode), mode_omega(mode), oracle(size, dtype, mode)
        for nt, remap in ((True, False), (False, True), (True, True)):
            tune = _tune(st, 5)
            tune.nontemporal, tune.xcd_remap = nt, remap
            info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om, tune=tune)
            if expect_fast is not None:
                cols = -(-(-(-size[0] // (4 if dtype == torch.float32 else 2))) // 64)  # wave columns of 64 16-B chunks
                assert (info["path"] == "fast") == expect_fast and info["blocks"] == cols * 3 * 4, info
            dd.next(0, qu).fill_(SENTINEL)
            _sync(dd)
            varcoef_relax(dd, 0, qu, qk, qf, w, omega=om, tune=tune)
            _sync(dd)
            got = dd.interior(dd.next(0, qu), 0).cpu()
            assert same_bits(got, want), _report(got, want, f"{mode} nontemporal {nt} xcd_remap {remap}")


# ---- 2. the new oracle against two the project already trusts ----
def case_oracle_identity(dtype, size=(23, 12, 16)):
    """the residual is 1 * f + (-1) * (A u): both products are exact, so the two oracles agree bit for bit"""
    u, k, f, w = global_u(size, dtype), global_kappa(size, dtype), global_f(size, dtype), random_weights()
    for walls in (None, "default"):
        bc, kbc = wall_conditions(walls)
        if bc is not None:
            kbc = mirror_twin(bc)
        want = axpby_reference(1.0, f, -1.0, varcoef_step_reference(u, k, w, boundary=bc, kappa_boundary=kbc))
        assert same_bits(varcoef_relax_reference(u, k, f, w, boundary=bc, kappa_boundary=kbc), want), walls


# ---- 3. destinations, and every byte outside the region ----
DST_SIZE = (37, 11, 9)
DESTINATIONS = ["next_u", "curr_v", "next_f", "curr_f"]


def _words(d, q, curr, word):
    raw = d.buffer_to_host(q, curr)
    assert len(raw) >= d.buffer_bytes(q) and len(raw) % np.dtype(word).itemsize == 0
    return np.frombuffer(raw, dtype=word)


def _cell_index(d, q, lo, hi):
    """element indices of the cells [lo, hi) (compute-region coordinates) in the raw allocation of quantity q"""
    p, r = d.pitch(q), d.radius()
    z = np.arange(lo[2], hi[2]).reshape(-1, 1, 1)
    y = np.arange(lo[1], hi[1]).reshape(1, -1, 1)
    x = np.arange(lo[0], hi[0]).reshape(1, 1, -1)
    return ((z + r.z(-1)) * p.y + (y + r.y(-1))) * p.x + d.pad_x(q) + r.x(-1) + x


def case_destination(st, backend, dtype, which, mode, expect_fast=None):
    """the sub-region "unaligned_x" into each allowed destination, whose whole allocation holds the fill byte first
    (in place: the fill byte around f's interior): afterwards the region holds the oracle and every other byte is
    what it was"""
    size = DST_SIZE
    lo, hi = sub_regions(size)["unaligned_x"]
    dd, qu, qk, qf, qv = make_domain(st, backend, size, dtype)
    d = dd.domain(0)
    word = np.uint32 if dtype == torch.float32 else np.uint64
    qd, curr = {"next_u": (qu, False), "curr_v": (qv, True), "next_f": (qf, False), "curr_f": (qf, True)}[which]
    d.fill_bytes(qd, FILL, curr, True)
    set_fields(dd, (qu, qk, qf), size, dtype)
    want = _words(d, qd, curr, word).copy()  # the fill, or the fill around f
    w, om = mode_weights(mode), mode_omega(mode)
    region = _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))
    tune = _tune(st, 4)
    info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om, dst=qd, dst_curr=curr, region=region, tune=tune)
    if expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    before = [_words(d, q, True, word).copy() for q in (qu, qk)]
    varcoef_relax(dd, 0, qu, qk, qf, w, omega=om, dst=qd, dst_curr=curr, region=region, tune=tune)
    _sync(dd)
    got = _words(d, qd, curr, word)
    idx = _cell_index(d, qd, lo, hi)
    ref = oracle(size, dtype, mode).numpy().view(word)
    want[idx] = ref[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    inside = np.zeros(got.shape, dtype=bool)
    inside[idx] = True
    diff = got != want
    assert int((diff & ~inside).sum()) == 0, f"{which}: {int((diff & ~inside).sum())} elements outside the region changed"
    assert int((diff & inside).sum()) == 0, f"{which}: {int((diff & inside).sum())} region cells differ from the oracle"
    for b, q, what in zip(before, (qu, qk), ("curr(u)", "curr(kappa)")):
        assert np.array_equal(b, _words(d, q, True, word)), f"{what} changed"


def case_refused_destinations(st, backend):
    """curr(u) and curr(kappa) are read at the neighbours: refused on the host, nothing is written"""
    size, dtype = (24, 12, 8), torch.float32
    dd, qu, qk, qf, _ = make_domain(st, backend, size, dtype)
    set_fields(dd, (qu, qk, qf), size, dtype)
    before = [dd.curr(0, q).cpu().clone() for q in (qu, qk)]
    for qd in (qu, qk):
        for om in (None, OMEGA):
            with pytest.raises(Exception, match="in place"):
                varcoef_relax(dd, 0, qu, qk, qf, jacobi_weights(), omega=om, dst=qd, dst_curr=True)
            with pytest.raises(Exception, match="in place"):
                varcoef_relax_launch_info(dd, 0, qu, qk, qf, jacobi_weights(), omega=om, dst=qd, dst_curr=True)
    _sync(dd)
    for b, q in zip(before, (qu, qk)):
        assert torch.equal(b, dd.curr(0, q).cpu())
    # their next buffers are fine
    varcoef_relax(dd, 0, qu, qk, qf, jacobi_weights(), omega=OMEGA, dst=qk, dst_curr=False)
    _sync(dd)
    assert same_bits(dd.interior(dd.next(0, qk), 0).cpu(), oracle(size, dtype, "jacobi"))


# ---- 4. sub-regions ----
def case_sub_region(st, backend, name, dtype, expect_fast=None):
    size = (37, 11, 9)
    lo, hi = sub_regions(size)[name]
    dd, qu, qk, qf, _ = make_domain(st, backend, size, dtype)
    set_fields(dd, (qu, qk, qf), size, dtype)
    region = _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))
    tune = _tune(st, 4)
    for mode in MODES:
        w, om = mode_weights(mode), mode_omega(mode)
        nxt = dd.next(0, qu)
        nxt.fill_(SENTINEL)
        _sync(dd)
        info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om, region=region, tune=tune)
        if name == "empty":
            assert info["path"] == "none", info
        elif expect_fast is not None:
            assert (info["path"] == "fast") == expect_fast, info
        varcoef_relax(dd, 0, qu, qk, qf, w, omega=om, region=region, tune=tune)
        _sync(dd)
        got = nxt.cpu()  # the whole raw tensor, halo included
        want = torch.full_like(got, SENTINEL)
        ref = oracle(size, dtype, mode)
        want[1 + lo[2]:1 + hi[2], 1 + lo[1]:1 + hi[1], 1 + lo[0]:1 + hi[0]] = ref[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        assert same_bits(got, want), _report(got, want, f"{name} {mode}")


# ---- 5. the unpadded layout and opaque elements ----
def case_generic_layout(st, backend, dtype):
    """an unpadded layout (rows of raw cells back to back, not 16-B aligned): the fast path refuses, one thread per
    cell computes the same"""
    size = (21, 9, 7)
    dd, qu, qk, qf, qv = make_domain(st, backend, size, dtype, padding=False)
    set_fields(dd, (qu, qk, qf), size, dtype)
    for mode in MODES:
        w, om = mode_weights(mode), mode_omega(mode)
        info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om, dst=qv, dst_curr=True)
        assert info["path"] == ("generic" if backend == _C.Backend.Device else "host"), info
        varcoef_relax(dd, 0, qu, qk, qf, w, omega=om, dst=qv, dst_curr=True)
        _sync(dd)
        got = dd.curr_interior(0, qv).cpu()
        assert same_bits(got, oracle(size, dtype, mode)), _report(got, oracle(size, dtype, mode), mode)


def case_opaque_bytes(st, backend, es):
    """opaque quantities of 4- / 8-byte elements are taken as fp32 / fp64, as varcoef_apply does"""
    size = (22, 12, 9)
    dtype = torch.float32 if es == 4 else torch.float64
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(1, 0, 0))
    dd.set_gpus([0])
    qu, qk, qf = (dd.native.add_data(es, n) for n in ("bu", "bk", "bf"))
    dd.realize()
    d = dd.domain(0)
    assert varcoef_relax_supported(dd, 0, qu, qk, qf)
    for q, g in ((qu, global_u(size, dtype)), (qk, global_kappa(size, dtype)), (qf, global_f(size, dtype))):
        d.region_from_host(_C.Dim3(1, 1, 1), d.size(), q, g.contiguous().numpy().tobytes(), True)
    dd.exchange()
    varcoef_relax(dd, 0, qu, qk, qf, jacobi_weights(), omega=OMEGA)
    dd.swap()
    _sync(dd)
    want = oracle(size, dtype, "jacobi")
    got = torch.from_numpy(np.frombuffer(d.interior_to_host(qu), dtype=want.numpy().dtype).reshape(tuple(want.shape)).copy())
    assert same_bits(got, want)


# ---- 6. a zero diagonal ----
def case_zero_diagonal(st, backend, dtype, expect_fast=None):
    """kappa = 0 and shift = 0: A u = 0 and the diagonal is 0, so the Jacobi sweep stores u + omega * (f / 0) = +-inf
    with the sign of f; not special-cased, bit for bit the oracle's"""
    size = (23, 12, 16)
    dd, qu, qk, qf, _ = make_domain(st, backend, size, dtype)
    u = global_u(size, dtype)
    f = global_f(size, dtype) - 0.5
    assert bool((f != 0).all()) and bool((f < 0).any()) and bool((f > 0).any())
    k = torch.zeros_like(u)
    set_fields(dd, (qu, qk, qf), size, dtype, kappa=k, f=f)
    w = varcoef_weights(0.0, -0.5, -0.25, -0.125)
    info = varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=OMEGA)
    if expect_fast is not None:
        assert (info["path"] == "fast") == expect_fast, info
    varcoef_relax(dd, 0, qu, qk, qf, w, omega=OMEGA)
    _sync(dd)
    got = dd.interior(dd.next(0, qu), 0).cpu()
    want = varcoef_relax_reference(u, k, f, w, omega=OMEGA)
    assert bool(torch.isinf(want).all()) and bool(((want > 0) == (f > 0)).all())
    assert same_bits(got, want), f"{int((got != want).sum())} cells differ"


# ---- 7. several sub-domains per GPU, walls: two ping-pong sweeps with an exchange between them ----
def make_pingpong(st, backend, size, dtype, gpus, axis_cost=None, walls=None):
    bc, kbc = wall_conditions(walls)
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(st.Radius.face_edge_corner(1, 0, 0))
    dd.set_gpus(list(gpus))
    if axis_cost is not None:
        dd.set_axis_cost(_C.Dim3(*axis_cost))
    qu, qk, qf, qv = (dd.add_data(n, dtype) for n in ("u", "kappa", "f", "v"))
    if bc is not None:
        dd.set_boundary_conditions(bc)  # u, v (and f, which is read at the centre only)
        dd.set_boundary_conditions(qk, kbc if kbc is not None else mirror_twin(bc))
    dd.realize()
    X, Y, Z = size
    for q, g in ((qu, global_u(size, dtype)), (qk, global_kappa(size, dtype)), (qf, global_f(size, dtype))):
        dd.fill_from_global(q, lambda gz, gy, gx, g=g: g.to(gz.device)[gz % Z, gy % Y, gx % X])
    return dd, bc, (qu, qk, qf, qv)


def gather(dd, q, dtype):
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=dtype)
    _sync(dd)
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = dd.curr_interior(di, q).cpu()
    return out


def case_pingpong(st, backend, size, gpus, dtype, axis_cost=None, walls=None):
    dd, bc, (qu, qk, qf, qv) = make_pingpong(st, backend, size, dtype, gpus, axis_cost, walls)
    assert dd.num_domains() == len(gpus)
    w = jacobi_weights()
    for src, dst in ((qu, qv), (qv, qu)):
        dd.exchange()
        if bc is not None:
            dd.apply_boundary()
        for di in range(dd.num_domains()):
            varcoef_relax(dd, di, src, qk, qf, w, omega=OMEGA, dst=dst, dst_curr=True)
    got, want = gather(dd, qu, dtype), oracle(size, dtype, "jacobi", 2, walls)
    assert same_bits(got, want), _report(got, want, f"two sweeps, walls {walls}")
    assert same_bits(gather(dd, qk, dtype), global_kappa(size, dtype)), "kappa changed"
    assert same_bits(gather(dd, qf, dtype), global_f(size, dtype)), "f changed"


WALL_SIZE = (24, 12, 10)


# ---- 8. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size = (24, 12, 8)
    w = jacobi_weights()
    dd, qu, qk, qf, qv = make_domain(st, backend, size, torch.float32,
                                     dtypes=[torch.float32, torch.float32, torch.float64, torch.float32])
    dd.next(0, qu).fill_(SENTINEL)
    _sync(dd)
    # f of another dtype
    assert not varcoef_relax_supported(dd, 0, qu, qk, qf)
    assert varcoef_relax_supported(dd, 0, qu, qk, qv)
    for om in (None, OMEGA):
        with pytest.raises(Exception, match="element size or row pitch"):
            varcoef_relax(dd, 0, qu, qk, qf, w, omega=om)
        with pytest.raises(Exception, match="element size or row pitch"):
            varcoef_relax_launch_info(dd, 0, qu, qk, qf, w, omega=om)
    # in-kernel wrap
    t = st.StencilTune()
    t.wrap = 1
    with pytest.raises(Exception, match="wrap"):
        varcoef_relax(dd, 0, qu, qk, qv, w, omega=OMEGA, tune=t)
    # a region outside the compute region; an empty one is a no-op
    with pytest.raises(Exception, match="outside compute region"):
        varcoef_relax(dd, 0, qu, qk, qv, w, omega=OMEGA, region=_C.Rect3(_C.Dim3(0, 0, 0), _C.Dim3(25, 12, 8)))
    whole = dd.domain(0).get_compute_region()
    assert varcoef_relax_launch_info(dd, 0, qu, qk, qv, w, region=_C.Rect3(whole.lo, whole.lo))["path"] == "none"
    varcoef_relax(dd, 0, qu, qk, qv, w, region=_C.Rect3(whole.lo, whole.lo))
    _sync(dd)
    assert bool((dd.next(0, qu) == SENTINEL).all())
    # a face radius of 0: one face short is enough
    r = st.Radius.face_edge_corner(1, 0, 0)
    r.set_dir(0, -1, 0, 0)
    dd0, qu0, qk0, qf0, _ = make_domain(st, backend, size, torch.float32, radius=r)
    dd0.next(0, qu0).fill_(SENTINEL)
    _sync(dd0)
    assert not varcoef_relax_supported(dd0, 0, qu0, qk0, qf0)
    with pytest.raises(Exception, match="face radii"):
        varcoef_relax(dd0, 0, qu0, qk0, qf0, w, omega=OMEGA)
    _sync(dd0)
    assert bool((dd0.next(0, qu0) == SENTINEL).all())
    # an unrealized domain has no sub-domain to apply to
    ddu = st.DistributedDomain(*size, group=st.make_single_group())
    ddu.set_backend(backend)
    ddu.add_data("u", torch.float32)
    with pytest.raises(Exception):
        varcoef_relax(ddu, 0, 0, 0, 0, w, region=whole)
