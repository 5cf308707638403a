"""Cases shared by test_transfer.py (host backend, the plain loops) and test_gpu_transfer.py (the HIP kernels of
csrc/src/kernels/grid_transfer.hip): restriction and prolongation between a fine DistributedDomain and its factor-2
coarse image, bitwise against ops.restrict_reference / ops.prolong_reference in fp32 and fp64.

Every launch is checked the same way (Pair.restrict / Pair.prolong): every byte of both buffers of every quantity of
the destination domain is first set to 0xAB, only the cells the call reads are written (for prolongation the coarse
interior, whose halos are then exchanged and filled by apply_boundary), all buffers of both domains are read back
whole before and after the call (row padding and tails included), and afterwards the region of dst must hold the
oracle's bits and every other byte of every buffer of both domains the bits it had before.

One refusal cannot be provoked with one GPU: sub-domains on different devices. Different backends stand in for it on
the device (test_gpu_transfer.py)."""
import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (grid_transfer_supported, prolong_apply, prolong_launch_info, prolong_reference,
                              restrict_apply, restrict_launch_info, restrict_reference)

import reduce_cases as rc
from reduce_cases import put, random_field, rect

FILL = 0xAB
DTYPES = [torch.float32, torch.float64]
dtype_id = rc.dtype_id
# fine (x, y, z): one chunk or less; coarse x off the chunk grid with odd coarse rows; a coarse row longer than one
# wave's chunks (261 cells: 66 fp32 / 131 fp64 chunks); more coarse rows than a block's four waves take
SHAPES = [(8, 2, 2), (2, 2, 2), (10, 6, 4), (522, 4, 4), (24, 70, 6)]
MARCH = ((16, 8, 40), 3)  # 20 coarse planes in z chunks of 3: seams at every third plane and a short last chunk
REGION_SIZE = (24, 12, 10)
# fine sub-regions that start and end on odd cells on every axis, a single cell, a single odd plane, an empty one
FINE_REGIONS = {
    "odd_all": ((3, 1, 1), (21, 11, 9)),
    "odd_start": ((1, 3, 5), (24, 12, 10)),
    "odd_end": ((0, 0, 0), (23, 11, 9)),
    "one_cell": ((7, 5, 3), (8, 6, 4)),
    "one_plane": ((0, 0, 5), (24, 12, 6)),
    "even_inner": ((8, 2, 2), (16, 10, 8)),
    "empty": ((4, 4, 4), (4, 9, 7)),
}
COARSE_REGIONS = {
    "inner": ((1, 1, 1), (11, 5, 4)),
    "off_chunk": ((3, 0, 0), (10, 6, 5)),
    "one_cell": ((5, 2, 3), (6, 3, 4)),
    "one_row": ((0, 3, 2), (12, 4, 3)),
    "empty": ((2, 2, 2), (2, 5, 4)),
}
# prolongation operands: add aliased with dst, add another quantity, add absent
ADDS = {"alias": "dst", "other": "b", "none": None}
# two sub-domains on GPU 0, cut along x, y, z in turn (the partition halves the longest axis)
CUTS = {"x": (32, 8, 8), "y": (8, 32, 8), "z": (8, 8, 32)}


def shape_id(s):
    return "x".join(map(str, s))


def np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def mixed_walls():
    """Constant, Mirror and AntiMirror on mixed faces: every edge and corner ghost cell composes two or three kinds"""
    FC = _C.FaceCondition
    bc = _C.BoundaryConditions()
    bc.set_axis(0, FC.constant(0.5), FC.mirror())
    bc.set_axis(1, FC.antimirror(1.0), FC.constant(-0.25))
    bc.set_axis(2, FC.mirror(), FC.antimirror(0.25))
    return bc


def field(size, dtype, seed, data="random"):
    u = random_field(tuple(size), dtype, seed)
    if data == "tiny":  # subnormal in both types: no flush to zero anywhere
        u = u * (1e-40 if dtype == torch.float32 else 1e-310)
        assert float(u.abs().max()) > 0
    return u


class Pair:
    """a fine domain with quantities a, b and its factor-2 coarse image with quantities c, d, all of one dtype"""

    def __init__(self, st, backend, fine_size, dtype, gpus=(0,), bc=None, padding=True, coarse_radius=None,
                 coarse_size=None, coarse_dtype=None, coarse_backend=None, extra_fine=(), realize=True):
        self.st, self.backend, self.dtype, self.bc = st, backend, dtype, bc
        self.fsize = tuple(fine_size)
        self.csize = tuple(coarse_size) if coarse_size is not None else tuple(v // 2 for v in fine_size)
        self.word = np.uint32 if dtype == torch.float32 else np.uint64
        self.fine = self._domain(self.fsize, backend, dtype, gpus, bc, padding, None)
        self.coarse = self._domain(self.csize, coarse_backend if coarse_backend is not None else backend,
                                   coarse_dtype or dtype, gpus, bc, padding, coarse_radius)
        self.q = {"a": (self.fine, self.fine.add_data("a", dtype)), "b": (self.fine, self.fine.add_data("b", dtype)),
                  "c": (self.coarse, self.coarse.add_data("c", coarse_dtype or dtype)),
                  "d": (self.coarse, self.coarse.add_data("d", coarse_dtype or dtype))}
        self.extra = [self.fine.add_data(f"x{i}", dt) for i, dt in enumerate(extra_fine)]
        if realize:
            self.fine.realize()
            self.coarse.realize()
            assert self.fine.num_domains() == self.coarse.num_domains() == len(gpus)

    def _domain(self, size, backend, dtype, gpus, bc, padding, radius):
        dd = self.st.DistributedDomain(*size, group=self.st.make_single_group())
        dd.set_backend(backend)
        dd.set_radius(radius if radius is not None else self.st.Radius.face_edge_corner(1, 1, 1))
        dd.set_gpus(list(gpus))
        if not padding:
            dd.set_padding(False)
        if bc is not None:
            dd.set_boundary_conditions(bc)
        return dd

    # ---- whole-buffer snapshots ----
    def buffers(self):
        rc.sync(self.fine)
        out = {}
        for name, (dd, q) in self.q.items():
            for di in range(dd.num_domains()):
                for curr in (True, False):
                    out[(name, di, curr)] = np.frombuffer(dd.domain(di).buffer_to_host(q, curr), dtype=self.word).copy()
        return out

    def fill(self, names):
        for name in names:
            dd, q = self.q[name]
            for di in range(dd.num_domains()):
                dd.domain(di).fill_bytes(q, FILL, True, True)
        rc.sync(self.fine)

    def clip(self, dd, di, lo, hi):
        """[lo, hi) cut to sub-domain di of dd (global coordinates), or None"""
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        l = (max(lo[0], o.x), max(lo[1], o.y), max(lo[2], o.z))
        h = (min(hi[0], o.x + s.x), min(hi[1], o.y + s.y), min(hi[2], o.z + s.z))
        return None if any(h[i] <= l[i] for i in range(3)) else (l, h)

    def index(self, dd, di, q, lo, hi):
        """element indices into buffer_to_host of the global cells [lo, hi) of sub-domain di"""
        d = dd.domain(di)
        p, ao = d.pitch(q), d.accessor_origin()
        z = np.arange(lo[2], hi[2]).reshape(-1, 1, 1) - ao.z
        y = np.arange(lo[1], hi[1]).reshape(1, -1, 1) - ao.y
        x = np.arange(lo[0], hi[0]).reshape(1, 1, -1) - ao.x
        return (z * p.y + y) * p.x + d.pad_x(q) + x

    def check(self, before, after, dst, lo, hi, want, what):
        """dst = (name, curr): its cells [lo, hi) hold `want` (the global tensor), everything else what it held"""
        dd, q = self.q[dst[0]]
        for key, old in before.items():
            expect = old
            if (key[0], key[2]) == dst:
                part = self.clip(dd, key[1], lo, hi)
                if part is not None:
                    l, h = part
                    expect = old.copy()
                    sub = want[l[2]:h[2], l[1]:h[1], l[0]:h[0]].contiguous().numpy().view(self.word)
                    expect[self.index(dd, key[1], q, l, h)] = sub
            diff = after[key] != expect
            assert not diff.any(), (f"{what}: buffer {key}: {int(diff.sum())} elements differ "
                                    f"(first at element {int(np.flatnonzero(diff)[0])})")

    # ---- the two transfers ----
    def restrict(self, src=("a", True), dst=("c", True), lo=(0, 0, 0), hi=None, data="random", device_path="fast",
                 seed=71):
        hi = self.csize if hi is None else tuple(hi)
        self.fill("abcd")
        F = field(self.fsize, self.dtype, seed, data)
        put(self.fine, self.q[src[0]][1], src[1], F)
        want = restrict_reference(F)
        before = self.buffers()
        empty = any(hi[i] <= lo[i] for i in range(3))
        infos = []
        for di in range(self.coarse.num_domains()):
            part = (lo, hi) if empty else self.clip(self.coarse, di, lo, hi)
            if part is None:
                continue
            args = (self.fine, self.coarse, di, self.q[src[0]][1], self.q[dst[0]][1])
            kw = dict(src_curr=src[1], dst_curr=dst[1], region=rect(*part))
            assert grid_transfer_supported(self.fine, self.coarse, di, args[3], args[4])
            info = restrict_launch_info(*args, **kw)
            assert info["path"] == ("none" if empty else rc.expected_path(self.backend, device_path)), info
            if not empty:
                assert info["items"] == (part[1][1] - part[0][1]) * (part[1][2] - part[0][2]), info
                if self.backend == _C.Backend.Device:
                    assert info["blocks"] >= 1, info
            restrict_apply(*args, **kw)
            infos.append(info)
        after = self.buffers()
        self.check(before, after, dst, lo, hi, want, f"restrict {self.fsize} {self.dtype} {src}->{dst} [{lo}, {hi}) {infos}")
        return infos

    def prolong(self, src=("c", True), dst=("a", True), add=None, lo=(0, 0, 0), hi=None, data="random",
                device_path="fast", zchunk=0, seed=81):
        hi = self.fsize if hi is None else tuple(hi)
        self.fill("abcd")
        C = field(self.csize, self.dtype, seed, data)
        put(self.coarse, self.q[src[0]][1], src[1], C)
        assert src[1], "the exchange fills the halos of curr"
        self.coarse.exchange()
        if self.bc is not None:
            self.coarse.apply_boundary(self.q[src[0]][1])
        A = None
        if add is not None:
            A = field(self.fsize, self.dtype, seed + 1, data)
            put(self.fine, self.q[add[0]][1], add[1], A, lo, hi)
        want = prolong_reference(C, boundary=self.bc, add=A)
        before = self.buffers()
        empty = any(hi[i] <= lo[i] for i in range(3))
        infos = []
        for di in range(self.fine.num_domains()):
            part = (lo, hi) if empty else self.clip(self.fine, di, lo, hi)
            if part is None:
                continue
            args = (self.coarse, self.fine, di, self.q[src[0]][1], self.q[dst[0]][1])
            kw = dict(add=None if add is None else self.q[add[0]][1], src_curr=src[1], dst_curr=dst[1],
                      add_curr=True if add is None else add[1], region=rect(*part), zchunk=zchunk)
            info = prolong_launch_info(*args, **kw)
            assert info["path"] == ("none" if empty else rc.expected_path(self.backend, device_path)), info
            if info["path"] == "fast":
                nk = (part[1][2] - 1) // 2 + 1 - part[0][2] // 2
                nj = (part[1][1] - 1) // 2 + 1 - part[0][1] // 2
                o = self.fine.domain(di).origin()
                V = 4 if self.dtype == torch.float32 else 2  # cells of a 16-B chunk; 64 chunks per wave item
                npass = -(-(-(-(part[1][0] - o.x) // V) - (part[0][0] - o.x) // V) // 64)
                zc = min(zchunk, nk) if zchunk else info["zchunk"]
                assert 1 <= zc <= nk and info["zchunk"] == zc, info
                assert info["items"] == npass * nj * -(-nk // zc) and info["blocks"] == -(-info["items"] // 4), info
            prolong_apply(*args, **kw)
            infos.append(info)
        after = self.buffers()
        self.check(before, after, dst, lo, hi, want,
                   f"prolong {self.fsize} {self.dtype} {src}->{dst} add {add} [{lo}, {hi}) zchunk {zchunk} {infos}")
        return infos


def add_operand(name, dst):
    return {"dst": dst, "b": ("b", True), None: None}[ADDS[name]]


# ---- 1. shapes ----
def case_shape(st, backend, size, dtype, zchunk=0):
    p = Pair(st, backend, size, dtype)
    p.restrict()
    p.restrict(src=("b", False), dst=("d", False))
    for name in ADDS:
        p.prolong(add=add_operand(name, ("a", True)), zchunk=zchunk)
    p.prolong(src=("d", True), dst=("b", False), add=("b", False), zchunk=zchunk)  # in place on next
    p.prolong(dst=("a", False), add=("a", True), zchunk=zchunk)  # the other buffer of one quantity
    return p


# ---- 2. sub-regions ----
def case_fine_region(st, backend, name, dtype, add):
    lo, hi = FINE_REGIONS[name]
    p = Pair(st, backend, REGION_SIZE, dtype)
    p.prolong(add=add_operand(add, ("a", True)), lo=lo, hi=hi, zchunk=2)


def case_coarse_region(st, backend, name, dtype):
    lo, hi = COARSE_REGIONS[name]
    Pair(st, backend, REGION_SIZE, dtype).restrict(lo=lo, hi=hi)


# ---- 3. layouts: the unpadded rows take one thread per cell ----
def case_unpadded(st, backend, dtype):
    p = Pair(st, backend, (10, 6, 4), dtype, padding=False)
    p.restrict(device_path="generic")
    lo, hi = (1, 1, 1), (9, 5, 3)
    for name in ADDS:
        p.prolong(add=add_operand(name, ("a", True)), device_path="generic")
        p.prolong(add=add_operand(name, ("a", True)), lo=lo, hi=hi, device_path="generic")


# ---- 4. two sub-domains: far cells from the other sub-domain's halo ----
def case_cut(st, backend, axis, dtype, bc=None):
    p = Pair(st, backend, CUTS[axis], dtype, gpus=(0, 0), bc=bc)
    ax = "xyz".index(axis)
    o = [p.fine.domain(di).origin() for di in range(2)]
    assert sorted((v.x, v.y, v.z)[ax] for v in o) == [0, CUTS[axis][ax] // 2], f"cut along {axis}: origins {o}"
    p.restrict()
    p.prolong(add=("a", True))
    p.prolong(lo=(1, 1, 1), hi=tuple(v - 1 for v in CUTS[axis]))


# ---- 5. walls: composed edge and corner ghost cells are consumed ----
def case_walls(st, backend, dtype, gpus=(0,)):
    p = Pair(st, backend, (12, 10, 8), dtype, gpus=gpus, bc=mixed_walls())
    p.prolong()
    p.prolong(add=("a", True))


# ---- 6. subnormal data ----
def case_tiny(st, backend, dtype):
    p = Pair(st, backend, (10, 6, 4), dtype)
    p.restrict(data="tiny")
    p.prolong(data="tiny")
    p.prolong(add=("a", True), data="tiny")


# ---- 7. refusals (all on the host, before any launch) ----
def case_refusals(st, backend):
    size, f32 = (8, 8, 8), torch.float32
    p = Pair(st, backend, size, f32, extra_fine=(torch.int32, torch.float64))
    qa, qb, qc, qd = (p.q[n][1] for n in "abcd")
    qi, q64 = p.extra
    R = [lambda *a, **k: restrict_apply(p.fine, p.coarse, *a, **k), lambda *a, **k: restrict_launch_info(p.fine, p.coarse, *a, **k)]
    P = [lambda *a, **k: prolong_apply(p.coarse, p.fine, *a, **k), lambda *a, **k: prolong_launch_info(p.coarse, p.fine, *a, **k)]
    for fn in R:
        with pytest.raises(Exception, match="fp32 / fp64"):
            fn(0, qi, qc)
        with pytest.raises(Exception, match="differ in type"):
            fn(0, q64, qc)
        for lo, hi in (((0, 0, 0), (5, 4, 4)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (4, 4, 5))):
            with pytest.raises(Exception, match="outside compute region"):
                fn(0, qa, qc, region=rect(lo, hi))
        with pytest.raises(Exception, match="no local sub-domain 1"):
            fn(1, qa, qc)
    for fn in P:
        with pytest.raises(Exception, match="fp32 / fp64"):
            fn(0, qc, qi)
        with pytest.raises(Exception, match="fp32 / fp64"):
            fn(0, qc, qa, add=qi)
        with pytest.raises(Exception, match="differ in type"):
            fn(0, qc, q64)
        with pytest.raises(Exception, match="differ in type"):
            fn(0, qc, qa, add=q64)
        for lo, hi in (((0, 0, 0), (9, 8, 8)), ((0, -1, 0), (8, 8, 8)), ((0, 0, 1), (8, 8, 9))):
            with pytest.raises(Exception, match="outside compute region"):
                fn(0, qc, qa, region=rect(lo, hi))
        with pytest.raises(Exception, match="zchunk"):
            fn(0, qc, qa, zchunk=-1)
    assert grid_transfer_supported(p.fine, p.coarse, 0, qa, qc) and grid_transfer_supported(p.fine, p.coarse, 0, qb, qd)
    assert not grid_transfer_supported(p.fine, p.coarse, 0, qi, qc)
    assert not grid_transfer_supported(p.fine, p.coarse, 0, q64, qc)
    # sizes and origins that are not the factor-2 image of each other
    # (the last: two sub-domains of 5 cells each along x are odd, whatever the coarse domain does)
    for fsize, csize, gpus in (((8, 8, 8), (4, 4, 8), (0,)), ((8, 8, 8), (8, 8, 8), (0,)), ((7, 8, 8), (3, 4, 4), (0,)),
                               ((10, 4, 4), (5, 2, 2), (0, 0))):
        bad = Pair(st, backend, fsize, f32, coarse_size=csize, gpus=gpus)
        a, c = bad.q["a"][1], bad.q["c"][1]
        di = bad.fine.num_domains() - 1
        assert not grid_transfer_supported(bad.fine, bad.coarse, di, a, c)
        r1 = rect((0, 0, 0), (1, 1, 1))
        for fn, args in ((restrict_apply, (bad.fine, bad.coarse, di, a, c)), (restrict_launch_info, (bad.fine, bad.coarse, di, a, c)),
                         (prolong_apply, (bad.coarse, bad.fine, di, c, a)), (prolong_launch_info, (bad.coarse, bad.fine, di, c, a))):
            with pytest.raises(Exception, match="factor-2 image"):
                fn(*args, region=r1)
    # different element types across the two domains
    mixed = Pair(st, backend, size, f32, coarse_dtype=torch.float64)
    a, c = mixed.q["a"][1], mixed.q["c"][1]
    assert not grid_transfer_supported(mixed.fine, mixed.coarse, 0, a, c)
    with pytest.raises(Exception, match="differ in type"):
        restrict_apply(mixed.fine, mixed.coarse, 0, a, c)
    with pytest.raises(Exception, match="differ in type"):
        prolong_launch_info(mixed.coarse, mixed.fine, 0, c, a)
    # prolongation reads all 26 coarse halo directions; restriction reads none
    faces = Pair(st, backend, size, f32, coarse_radius=st.Radius.face_edge_corner(1, 1, 0))
    a, c = faces.q["a"][1], faces.q["c"][1]
    for fn in (prolong_apply, prolong_launch_info):
        with pytest.raises(Exception, match="26 directions"):
            fn(faces.coarse, faces.fine, 0, c, a)
    assert restrict_launch_info(faces.fine, faces.coarse, 0, a, c)["path"] != "none"
    # an unrealized domain has no sub-domain to take
    und = Pair(st, backend, size, f32, realize=False)
    a, c = und.q["a"][1], und.q["c"][1]
    r1 = rect((0, 0, 0), (1, 1, 1))
    for fn, args in ((restrict_apply, (und.fine, und.coarse, 0, a, c)), (restrict_launch_info, (und.fine, und.coarse, 0, a, c)),
                     (prolong_apply, (und.coarse, und.fine, 0, c, a)), (prolong_launch_info, (und.coarse, und.fine, 0, c, a))):
        with pytest.raises(Exception, match="no local sub-domain 0"):
            fn(*args, region=r1)
    und.fine.realize()  # one of the two realized is still refused
    with pytest.raises(Exception, match="no local sub-domain 0"):
        restrict_apply(und.fine, und.coarse, 0, a, c, region=r1)
    # the refusals come before anything is written
    p.fill("abcd")
    before = p.buffers()
    with pytest.raises(Exception, match="outside compute region"):
        prolong_apply(p.coarse, p.fine, 0, qc, qa, region=rect((0, 0, 0), (8, 8, 9)))
    after = p.buffers()
    assert all((before[k] == after[k]).all() for k in before)


def case_backends_differ(st):
    """a device sub-domain and a host sub-domain are no pair (stands in for two devices, which one GPU cannot show)"""
    p = Pair(st, _C.Backend.Device, (8, 8, 8), torch.float32, coarse_backend=_C.Backend.Host)
    a, c = p.q["a"][1], p.q["c"][1]
    assert not grid_transfer_supported(p.fine, p.coarse, 0, a, c)
    for fn, args in ((restrict_apply, (p.fine, p.coarse, 0, a, c)), (restrict_launch_info, (p.fine, p.coarse, 0, a, c)),
                     (prolong_apply, (p.coarse, p.fine, 0, c, a)), (prolong_launch_info, (p.coarse, p.fine, 0, c, a))):
        with pytest.raises(Exception, match="different backends"):
            fn(*args)
