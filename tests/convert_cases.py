"""Cases shared by test_convert.py (host backend, the plain loop) and test_gpu_convert.py (the HIP kernels of
csrc/src/kernels/field_convert.hip): dst = T_dst(scale * double(src)) between two domains of one compute region,
bitwise against ops.convert_reference for the four type pairs, the stats of the stored values fused into the same pass
and DistributedDomain.convert_from.

Every launch is checked the same way (Pair.run): every byte of both buffers of every quantity of both domains is first
set to 0xAB, only the source cells of the region are written, all buffers are read back whole before and after the call
(halos, row padding and tails included), and afterwards the region of the destination must hold the oracle's bits and
every other byte of both domains the bits it had before. NaN payloads are not part of the contract: a cell that is NaN
on both sides counts as equal.

The two domains of a Pair differ in radius (face_edge_corner(1, 1, 1) for the source, (3, 0, 0) for the destination)
unless a case says otherwise, so their pitches, plane sizes and interior offsets differ in every launch."""
import math

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (convert_reference, field_axpby, field_axpby_launch_info, field_convert,
                              field_convert_launch_info, field_convert_supported, field_reduce, field_reduce_launch_info)

import reduce_cases as rc
from reduce_cases import exact_field, put, random_field, rect

FILL = 0xAB
F32, F64 = torch.float32, torch.float64
PAIRS = [(F32, F64), (F64, F32), (F32, F32), (F64, F64)]
SCALES = [1, -0.375, 1 / 3, 1e-30, 1e30]
DATA = ["random", "subnormal", "overflow", "bits"]
# (8, 2, 2): one lane-item per row pair; (2, 2, 2): less than one item; (10, 6, 4): head and tail off the 4-cell grid
# (with the sub-regions); (522, 4, 4): a row longer than one wave's 64 items; (24, 70, 6): more rows than a block's waves
SHAPES = [(8, 2, 2), (2, 2, 2), (10, 6, 4), (522, 4, 4), (24, 70, 6)]
REGION_SIZE = (24, 12, 10)
REGIONS = {
    "odd_start_and_end": ((3, 1, 1), (21, 11, 7)),
    "head_only": ((5, 0, 0), (24, 12, 10)),
    "tail_only": ((0, 0, 0), (18, 12, 10)),
    "inside_one_item": ((13, 2, 3), (15, 9, 8)),
    "one_cell": ((9, 5, 2), (10, 6, 3)),
    "one_plane": ((0, 0, 3), (24, 12, 4)),
    "empty": ((4, 4, 4), (4, 9, 7)),
}
# the cut axis of two sub-domains follows the longest extent
CUTS = {"x": (48, 6, 4), "y": (10, 44, 4), "z": (10, 6, 40)}


def pair_id(p):
    return f"{rc.dtype_id(p[0])}_to_{rc.dtype_id(p[1])}"


def np_dtype(dtype):
    return np.float32 if dtype == F32 else np.float64


def word(dtype):
    return np.uint32 if dtype == F32 else np.uint64


def source(size, dtype, dst_dtype, scale, kind, seed=71):
    """a (z, y, x) source field of `dtype`. "random": uniform [-1, 1); "subnormal" / "overflow": scale * source lands
    among the subnormals of the destination type / around and beyond the largest fp32 (as far as the source type can
    hold such values: the rest saturates to 0 or Inf, which converts like anything else); "bits": uniformly random bit
    patterns, so every exponent, subnormals, +-Inf and NaNs, plus planted +-0, +-Inf, NaN, the largest and the
    smallest magnitudes"""
    X, Y, Z = size
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return random_field(tuple(size), dtype, seed)
    if kind == "bits":
        es = 4 if dtype == F32 else 8
        u = torch.randint(0, 256, (Z, Y, X * es), generator=g, dtype=torch.uint8).view(dtype).clone()
        fi = torch.finfo(dtype)
        special = [0.0, -0.0, math.inf, -math.inf, math.nan, fi.max, -fi.max, fi.tiny, fi.tiny * fi.eps, 3.5e38, 1e-45]
        flat = u.view(-1)
        sp = torch.tensor(special, dtype=F64).to(dtype)[:flat.numel()]  # what the type cannot hold saturates
        flat[(torch.arange(sp.numel()) * 7) % flat.numel()] = sp
        return u
    t = torch.rand((Z, Y, X), generator=g, dtype=F64) * 2 - 1
    if kind == "subnormal":
        t = t * torch.finfo(dst_dtype).tiny
    else:
        assert kind == "overflow", kind
        t = t * 4 * torch.finfo(F32).max
    return (t / float(scale)).to(dtype)


def make(st, backend, size, radius, gpus=(0,), **layout):
    """a domain with two fp32 quantities, two fp64 quantities and an int32 one: {dtype: (q, q)}, qi"""
    dd, a32, b32, (a64, b64, qi) = rc.make_domain(st, backend, size, F32, gpus=gpus, radius=radius,
                                                  extra=(F64, F64, torch.int32), **layout)
    return dd, {F32: (a32, b32), F64: (a64, b64)}, qi


class Pair:
    """a source and a destination domain of one size (same=True: one domain on both sides), reused by the launches of
    a test"""

    def __init__(self, st, backend, size, same=False, gpus=(0,), src_layout=None, dst_layout=None):
        self.st, self.backend, self.size = st, backend, tuple(size)
        R = st.Radius.face_edge_corner
        self.src, self.sq, _ = make(st, backend, size, R(1, 1, 1), gpus, **(src_layout or {}))
        if same:
            self.dst, self.dq = self.src, self.sq
        else:
            self.dst, self.dq, _ = make(st, backend, size, R(3, 0, 0), gpus, **(dst_layout or {}))
        self.dds = [self.src] if same else [self.src, self.dst]
        self.same = same
        self.nd = self.src.num_domains()
        assert self.nd == len(gpus) == self.dst.num_domains()

    def buffers(self):
        for dd in self.dds:
            rc.sync(dd)
        out = {}
        for k, dd in enumerate(self.dds):
            for di in range(self.nd):
                d = dd.domain(di)
                for q in range(d.num_data()):
                    for c in (True, False):
                        out[(k, di, q, c)] = np.frombuffer(d.buffer_to_host(q, c), dtype=np.uint8).copy()
        return out

    def fill(self):
        for dd in self.dds:
            for di in range(self.nd):
                d = dd.domain(di)
                for q in range(d.num_data()):
                    d.fill_bytes(q, FILL, True, True)

    @staticmethod
    def local(d, lo, hi):
        """[lo, hi) cut to the compute region of sub-domain d (global coordinates), or None"""
        o, s = d.origin(), d.size()
        l = (max(lo[0], o.x), max(lo[1], o.y), max(lo[2], o.z))
        h = (min(hi[0], o.x + s.x), min(hi[1], o.y + s.y), min(hi[2], o.z + s.z))
        return None if any(h[i] <= l[i] for i in range(3)) else (l, h)

    @staticmethod
    def index(d, q, l, h):
        """element indices of the global cells [l, h) in a buffer of quantity q of sub-domain d"""
        p, r, o = d.pitch(q), d.radius(), d.origin()
        z = np.arange(l[2], h[2]).reshape(-1, 1, 1) - o.z + r.z(-1)
        y = np.arange(l[1], h[1]).reshape(1, -1, 1) - o.y + r.y(-1)
        x = np.arange(l[0], h[0]).reshape(1, 1, -1) - o.x + r.x(-1)
        return (z * p.y + y) * p.x + d.pad_x(q) + x

    def run(self, sdt, ddt, scale, data="random", src_curr=True, dst_curr=True, lo=(0, 0, 0), hi=None, which=0,
            device_path="fast", u=None, collective=False, **kw):
        """field_convert of [lo, hi) on every sub-domain that holds some of it (collective: dst.convert_from over the
        compute regions) with the byte check of the module docstring. Source quantity: the first of its type; the
        destination the `which`-th of its type (same domain and type: the second). Returns (what the last call
        returned, its launch info, the oracle's region)"""
        hi = self.size if hi is None else tuple(hi)
        qs = self.sq[sdt][0]
        qd = self.dq[ddt][1 if self.same and sdt == ddt and src_curr == dst_curr else which]
        self.fill()
        if u is None:
            u = source(self.size, sdt, ddt, scale, data)
        put(self.src, qs, src_curr, u, lo, hi)
        before = self.buffers()
        sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        want = convert_reference(u[sl], scale, ddt)
        empty = any(hi[i] <= lo[i] for i in range(3))
        out = info = None
        args = dict(scale=scale, src_curr=src_curr, dst_curr=dst_curr)
        if collective:
            assert lo == (0, 0, 0) and hi == self.size
            out = self.dst.convert_from(self.src, qd, qs, stats=kw.get("stats", False), **args)
        else:
            for di in range(self.nd):
                box = (lo, hi) if empty else self.local(self.dst.domain(di), lo, hi)
                if box is None:
                    continue
                region = rect(*box)
                info = field_convert_launch_info(self.src, self.dst, di, qs, qd, region=region, **args, **kw)
                assert info["path"] == ("none" if empty else rc.expected_path(self.backend, device_path)), info
                if not empty:
                    assert info["items"] == (box[1][1] - box[0][1]) * (box[1][2] - box[0][2]), info
                    if self.backend == _C.Backend.Device:
                        mb = kw.get("max_blocks", 0)
                        assert info["blocks"] == mb if mb else 1 <= info["blocks"] <= info["items"], info
                assert field_convert_supported(self.src, self.dst, di, qs, qd)
                out = field_convert(self.src, self.dst, di, qs, qd, region=region, **args, **kw)
        after = self.buffers()
        what = f"{self.size} {sdt}->{ddt} scale={scale} {data} src_curr={src_curr} dst_curr={dst_curr} [{lo}, {hi}) {kw} {info}"
        kdst = len(self.dds) - 1
        f, w = np_dtype(ddt), word(ddt)
        for key, old in before.items():
            expect, got = old, after[key]
            if key[0] == kdst and key[2] == qd and key[3] == dst_curr and not empty:
                d = self.dst.domain(key[1])
                box = self.local(d, lo, hi)
                expect, got = old.view(w).copy(), got.view(w)
                if box is not None:
                    l, h = box
                    part = want[l[2] - lo[2]:h[2] - lo[2], l[1] - lo[1]:h[1] - lo[1], l[0] - lo[0]:h[0] - lo[0]]
                    expect[self.index(d, qd, l, h)] = part.contiguous().numpy().view(w)
                diff = (got != expect) & ~(np.isnan(got.view(f)) & np.isnan(expect.view(f)))
            else:
                diff = got != expect
            assert not diff.any(), (f"{what}: buffer {key}: {int(diff.sum())} elements differ "
                                    f"(first at element {int(np.flatnonzero(diff)[0])})")
        return out, info, want


# ---- 1. bitwise over shapes, type pairs, scales and data ----
def case_shape(st, backend, size, pair):
    p = Pair(st, backend, size)
    for scale in SCALES:
        for data in DATA:
            assert p.run(pair[0], pair[1], scale, data)[0] is None


def case_buffers(st, backend, pair):
    """curr and next on both sides, between two domains and within one"""
    for same in (False, True):
        p = Pair(st, backend, (10, 6, 4), same=same)
        for sc in (True, False):
            for dc in (True, False):
                p.run(pair[0], pair[1], -0.375, src_curr=sc, dst_curr=dc)
                p.run(pair[0], pair[1], 1, "bits", src_curr=sc, dst_curr=dc, stats=True)
        if same and pair[0] == pair[1]:
            # the two buffers of one quantity are taken (the same buffer is refused: case_refusals)
            q = p.sq[pair[0]][0]
            assert field_convert_launch_info(p.src, p.src, 0, q, q, src_curr=True, dst_curr=False)["path"] != "none"


# ---- 2. untouched bytes over sub-regions ----
def case_region(st, backend, name, pair, stats):
    lo, hi = REGIONS[name]
    p = Pair(st, backend, REGION_SIZE)
    out, info, _ = p.run(pair[0], pair[1], 1 / 3, lo=lo, hi=hi, stats=stats)
    p.run(pair[0], pair[1], 1, "bits", lo=lo, hi=hi, stats=stats, dst_curr=False)
    if name == "empty":
        assert info["path"] == "none" and (rc.fields(out) == rc.IDENTITY if stats else out is None)


# ---- 3. layouts ----
def case_unpadded(st, backend, side, pair):
    """set_padding(False) on either side: one thread per cell"""
    lay = dict(padding=False)
    p = Pair(st, backend, (37, 11, 9), src_layout=lay if side == "src" else None, dst_layout=lay if side == "dst" else None)
    p.run(pair[0], pair[1], -0.375, device_path="generic")
    p.run(pair[0], pair[1], 1, "bits", lo=(3, 1, 2), hi=(35, 10, 8), device_path="generic", stats=True)


def case_layout(st, backend, name, pair):
    """the layouts of reduce_cases.LAYOUTS on the destination side"""
    kw, path = rc.LAYOUTS[name]
    kw = dict(kw)
    kw.pop("radius", None)
    p = Pair(st, backend, (37, 11, 9), dst_layout=kw)
    p.run(pair[0], pair[1], 1 / 3, device_path=path)
    p.run(pair[0], pair[1], 1, "bits", lo=(3, 1, 2), hi=(35, 10, 8), device_path=path, stats=True)


# ---- 4. two sub-domains on one GPU ----
def case_cut(st, backend, axis, pair):
    size = CUTS[axis]
    p = Pair(st, backend, size, gpus=(0, 0))
    dim = p.dst.placement_dim()
    assert (dim.x, dim.y, dim.z) == tuple(2 if a == axis else 1 for a in "xyz"), dim
    p.run(pair[0], pair[1], -0.375)
    lo, hi = (1, 1, 1), tuple(v - 1 for v in size)
    p.run(pair[0], pair[1], 1e30, "overflow", lo=lo, hi=hi, dst_curr=False)
    out, _, want = p.run(pair[0], pair[1], 1 / 3, collective=True)
    assert out is None
    A = exact_field(size, 21)
    out, _, want = p.run(pair[0], pair[1], -3, u=A.to(pair[0]), collective=True, stats=True)
    rc.check_exact(out, rc.expect_exact(-3 * A), f"convert_from stats, cut along {axis}")
    qd = p.dq[pair[1]][0]
    assert rc.fields(p.dst.reduce(qd)) == rc.fields(out)


# ---- 5. fused stats ----
def case_stats_exact(st, backend, size, pair, max_blocks=0):
    p = Pair(st, backend, size)
    A = exact_field(tuple(size), 23)
    got, info, want = p.run(pair[0], pair[1], -2, u=A.to(pair[0]), stats=True, max_blocks=max_blocks)
    rc.check_exact(got, rc.expect_exact(-2 * A), f"{size} {pair} blocks {max_blocks} {info}")
    assert rc.fields(got) == rc.fields(field_reduce(p.dst, 0, p.dq[pair[1]][0]))
    return got


def case_forced_grid(st, backend, size, pair, max_blocks):
    auto = case_stats_exact(st, backend, size, pair)
    forced = case_stats_exact(st, backend, size, pair, max_blocks)
    assert rc.fields(auto) == rc.fields(forced), (rc.fields(auto), rc.fields(forced))
    p = Pair(st, backend, size)
    assert p.run(pair[0], pair[1], 1 / 3, max_blocks=max_blocks)[0] is None


def case_stats_random(st, backend, pair):
    """each sum within 2 n 2^-53 sum |t_i| of math.fsum of the oracle's terms (reduce_cases.case_random's any-order
    summation bound); min / max exact; the same struct as field_reduce of the destination within the same bound"""
    p = Pair(st, backend, rc.RANDOM_SIZE)
    got, _, want = p.run(pair[0], pair[1], -0.7, stats=True)
    v = want.numpy().astype(np.float64).ravel()
    n = v.size
    red = field_reduce(p.dst, 0, p.dq[pair[1]][0])
    assert got.count == n and got.nonfinite == 0 and got.dot == 0, rc.fields(got)
    for k, t in {"sum": v, "sum_abs": np.abs(v), "sum_sq": v * v}.items():
        ref, mag = math.fsum(t), math.fsum(np.abs(t))
        bound = 2 * n * 2.0 ** -53 * mag
        for name, s in (("convert", got), ("reduce", red)):
            err = abs(getattr(s, k) - ref)
            print(f"{k} ({name}): got {getattr(s, k)!r} ref {ref!r} err {err:.3e} bound {bound:.3e}")
            assert err <= bound, f"{k} ({name}): |{getattr(s, k)!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
    assert got.min == v.min() == red.min and got.max == v.max() == red.max, (rc.fields(got), v.min(), v.max())


def case_stats_nonfinite(st, backend, pair):
    """the NaNs and Infs of the random bit patterns (and those an fp32 destination overflows to) are counted"""
    p = Pair(st, backend, (37, 11, 9))
    got, _, want = p.run(pair[0], pair[1], 1, "bits", stats=True)
    nf = int((~torch.isfinite(want)).sum())
    assert nf >= 3 and got.count == want.numel() and got.nonfinite == nf and math.isnan(got.sum), (nf, rc.fields(got))
    assert got.max == math.inf and got.min == -math.inf, rc.fields(got)


def case_stats_repeatable(st, backend, pair):
    p = Pair(st, backend, rc.RANDOM_SIZE)
    outs = [rc.bits(p.run(pair[0], pair[1], 1 / 3, stats=True)[0]) for _ in range(2)]
    assert outs[0] == outs[1], [o.hex() for o in outs]


# ---- 6. launch info and refusals (all on the host, before any launch) ----
def case_launch_info(st, backend):
    p = Pair(st, backend, (24, 12, 8))
    for sdt, ddt in PAIRS:
        info = field_convert_launch_info(p.src, p.dst, 0, p.sq[sdt][0], p.dq[ddt][0])
        assert info["path"] == rc.expected_path(backend, "fast") and info["items"] == 12 * 8, info
        assert (info["blocks"] >= 1) == (backend == _C.Backend.Device), info
    q = p.sq[F32][0]
    assert field_convert_launch_info(p.src, p.dst, 0, q, p.dq[F64][0], max_blocks=3)["blocks"] == \
        (3 if backend == _C.Backend.Device else 0)


def case_refusals(st, backend):
    size = (24, 12, 8)
    p = Pair(st, backend, size)
    src, dst, sq, dq = p.src, p.dst, p.sq, p.dq
    qi = src.domain(0).num_data() - 1  # the int32 quantity (every domain of `make` has it last)
    other, oq, _ = make(st, backend, (24, 12, 10), st.Radius.face_edge_corner(1, 1, 1))
    two, tq, _ = make(st, backend, size, st.Radius.face_edge_corner(1, 1, 1), gpus=(0, 0))
    und = st.DistributedDomain(*size, group=st.make_single_group())
    und.set_backend(backend)
    u0 = und.add_data("a", F32)
    p.fill()
    before = p.buffers()
    a, b = sq[F32][0], dq[F64][0]
    for fn in (field_convert, field_convert_launch_info):
        for args in ((src, dst, 0, qi, b), (src, dst, 0, a, qi)):
            with pytest.raises(Exception, match="fp32 / fp64"):
                fn(*args)
        with pytest.raises(Exception, match="compute region"):
            fn(other, dst, 0, oq[F32][0], b, region=rect((0, 0, 0), (1, 1, 1)))
        with pytest.raises(Exception, match="compute region"):
            fn(src, two, 0, a, tq[F64][0], region=rect((0, 0, 0), (1, 1, 1)))  # half of the grid against the whole
        for lo, hi in (((0, 0, 0), (25, 12, 8)), ((-1, 0, 0), (24, 12, 8)), ((0, 0, 0), (24, 12, 9)), ((0, 13, 0), (24, 14, 8))):
            with pytest.raises(Exception, match="outside compute region"):
                fn(src, dst, 0, a, b, region=rect(lo, hi))
        for args in ((und, dst, 0, u0, b), (src, und, 0, a, u0)):
            with pytest.raises(Exception, match="unrealized"):
                fn(*args, region=rect((0, 0, 0), (1, 1, 1)))
        for curr in (True, False):
            with pytest.raises(Exception, match="same buffer"):
                fn(src, src, 0, a, a, src_curr=curr, dst_curr=curr)
        for mb in (-1, (1 << 20) + 1):
            with pytest.raises(Exception, match="maxBlocks"):
                fn(src, dst, 0, a, b, max_blocks=mb)
        for di in (1, 7):
            with pytest.raises(Exception):
                fn(src, dst, di, a, b)
    if backend == _C.Backend.Device:
        host, hq, _ = make(st, _C.Backend.Host, size, st.Radius.face_edge_corner(1, 1, 1))
        for fn in (field_convert, field_convert_launch_info):
            with pytest.raises(Exception, match="backend"):
                fn(host, dst, 0, hq[F32][0], b)
            with pytest.raises(Exception, match="backend"):
                fn(src, host, 0, a, hq[F64][0])
    assert not field_convert_supported(src, dst, 0, qi, b) and not field_convert_supported(other, dst, 0, oq[F32][0], b)
    assert all(field_convert_supported(src, dst, 0, sq[s][0], dq[d][0]) for s, d in PAIRS)
    with pytest.raises(Exception, match="realize"):
        dst.convert_from(und, b, u0)
    with pytest.raises(Exception, match="sub-domains"):
        dst.convert_from(two, b, tq[F32][0])
    with pytest.raises(Exception, match="fp32 / fp64"):
        dst.convert_from(src, b, qi)
    after = p.buffers()
    assert all((before[k] == after[k]).all() for k in before), "a refused call wrote"
    # the kernels of one type still refuse two
    for fn in (field_axpby, field_axpby_launch_info):
        with pytest.raises(Exception, match="differ in type"):
            fn(src, 0, sq[F32][0], 1.0, sq[F64][0])
    with pytest.raises(Exception):
        field_reduce(src, 0, sq[F32][0], other=sq[F64][0])
    with pytest.raises(Exception):
        field_reduce_launch_info(src, 0, sq[F32][0], other=sq[F64][0])
