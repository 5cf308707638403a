"""Cases shared by test_stencil7_regions.py (host backend) and test_gpu_stencil7_regions.py (the HIP kernels): the
single 7-point step (csrc/src/kernels/stencil7.hip, stencil7_mfma.hip) and the fused pair (stencil7x2.hip) launched
directly, per region, kernel form and StencilTune.

Every case goes through one check (`prepare` + `check_buffer`): the whole `next` buffer is filled with one byte value,
curr is exchanged (and the halos of in-kernel wrapped axes overwritten with NaN), the call runs, and the whole
allocation of `next` is read back. Every cell of the region(s) must equal the torch CPU oracle bitwise (compared as
integers) and every other byte of the allocation -- halos, row padding, front slack, compute cells outside the region --
must still hold the fill byte. The two counts are reported separately.

What launches what (A = single step, B = fused pair):

  kernel instance / path                                   case
  -------------------------------------------------------  ----------------------------------------------------------
  stencil7_lds_kernel PF 2, ty 2, nw 8 (the default)       A shapes / sub-regions, instance v2-ty2-nw8
  stencil7_lds_kernel PF 1 (variant 0) ty 2 / 4 / 8        A shapes / sub-regions, instances v0-ty2, v0-ty4, v0-ty8
  variant 0, nontemporal False / xcd_remap False           A instances v0-ty2-plain-stores, v0-ty2-no-remap
  stencil7_kernel (variant 1) ty 4 / 8                     A instances v1-ty4, v1-ty8
  stencil7_kernel, nontemporal and xcd_remap False         A instance v1-ty8-plain-no-remap
  variant 2 with ty 1; nw 4; nw 16                         A instances v2-ty1, v2-nw4, v2-nw16
  variants 3 and 4 (3 / 4 planes of lookahead)             A instances v3, v4
  explicit zchunk (seams, odd chunks marching down,        A shapes (24,12,17) zchunk 5, (24,12,9) zchunk 1, the
    a short last chunk), the automatic chunk                 sub-regions (zchunk 4), (24,12,40) automatic
  alternate_z on the odd parity                            case_single_parity / case_pair_parity
  stencil7_mfma_kernel, partial 64x16 tiles, zchunk        MFMA_SHAPES, case_single_sub_region with the MFMA instance
  stencil7_generic_kernel (unpadded layout)                case_single_layout("unpadded")
  shared halo lines (x = 96), interior_align(64)           case_single_layout("shared_halo_line" / "align64")
  stencil7_lds_kernel WRAP, masks 1-7                      case_single_wrap (whole region and sub-ranges)
  stencil7_shell_kernel row / column mode, table loop      case_single_regions: shell1-3, width7and8, many9, many17
  stencil7_regions_kernel (unpadded layout), table loop    case_single_regions(..., padded=False)
  stencil7_shell_kernel wrap 6                             case_single_regions("wrap6_x_slabs")
  host_apply, host path of stencil7_apply_regions          test_stencil7_regions.py (the same cases on Backend.Host)
  stencil7x2_kernel (column form) x2sched 0 / 1, zchunk    B PAIR_COLUMN_SHAPES x PAIR_SCHEDS, the pair sub-regions
  column form, x2xfast 0 / 1 (x = 513: 3 block columns)    case_pair_shape(..., xfast)
  row forms row / ragged2 / ragged3 / tail, wrap 1 3 5 7   PAIR_ROW_CASES (x2early both ways, y / z sub-ranges)
  stencil7x2_col2_kernel, wrap 0 / 2 / 4 / 6, x sub-range  PAIR_COL2_CASES
  stencil7x2_thin_kernel <= 2 and 3-4 cells, per axis      case_pair_exterior shrink 1-4, unequal shrinks, wrap 1 2 4
  stencil7x2_regions_kernel, table loop                    case_pair_exterior shrink 5, case_pair_regions 9 / 17
  refusals (message, and `next` keeps its fill)            case_single_refusals / case_pair_refusals
"""
import functools

import numpy as np
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (astaroth_step_reference, jacobi_step_reference, stencil7_apply, stencil7_apply_regions,
                              stencil7_wrappable_axes, stencil7x2_apply, stencil7x2_apply_exterior,
                              stencil7x2_apply_regions, stencil7x2_launch_info, stencil7x2_wrappable_axes)
from star_cases import SHAPES, sub_regions

FILL = 0xAB
KINDS = ["astaroth", "jacobi"]
DTYPES = [torch.float32, torch.float64]
SUB_SIZE = (37, 11, 9)  # Jacobi: radius 3, centres (12, 5, 4) and (24, 5, 4): inside the grid, cut by the sub-regions


def dtype_id(dt):
    return str(dt).split(".")[-1]


def kind_of(name):
    return _C.StencilKind.Jacobi if name == "jacobi" else _C.StencilKind.Astaroth


# ---- the oracle: torch on the CPU, in the quantity's dtype ----
@functools.lru_cache(maxsize=None)
def global_field(size, dtype, seed=5):
    X, Y, Z = size
    return torch.rand((Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=dtype)


@functools.lru_cache(maxsize=None)
def oracle(size, dtype, kind, steps=1):
    """`steps` reference steps of the case's field, as unsigned integer words (z, y, x); shared, never modified"""
    u = global_field(size, dtype)
    assert u.device.type == "cpu"
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    for _ in range(steps):
        u = ref(u)
    assert u.dtype == dtype and bool(((u >= 0) & (u <= 1)).all())
    w = u.contiguous().numpy().view(np.uint32 if dtype == torch.float32 else np.uint64)
    w.setflags(write=False)
    return w


def case_oracle_against_fp64(kind):
    """the fp32 oracle against the fp64 evaluation of the same field: for values in [0, 1) five rounded additions of
    partial sums below 8 contribute at most 5 * 2^-22 / 6 after the division, the quotient's rounding at most 2^-25"""
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    worst = 0.0
    for size in ((37, 11, 9), (24, 12, 17), (257, 12, 16)):
        u = global_field(size, torch.float32)
        got = ref(u).to(torch.float64)
        want = ref(u.to(torch.float64))
        err = (got - want).abs().max().item()
        worst = max(worst, err)
        assert err <= 2.0 ** -22, (size, err)
        if kind == "jacobi":  # the spheres are there, exact in both
            assert int((got == 1).sum()) > 0 and int((got == 0).sum()) > 0
    assert worst > 0  # the two are not the same computation
    return worst


# ---- domains ----
class Dom:
    """one single-sub-domain DistributedDomain with its quantity and what the check needs of its layout"""

    def __init__(self, st, backend, size, radius, dtype, layout="padded"):
        dd = st.DistributedDomain(*size, group=st.make_single_group())
        dd.set_backend(backend)
        dd.set_radius(radius)
        dd.set_gpus([0])
        if layout == "unpadded":
            dd.set_padding(False)
        elif layout == "shared_halo_line":
            dd.set_shared_halo_line(True)
        elif layout == "align64":
            dd.set_interior_align(64)
        else:
            assert layout == "padded", layout
        self.q = dd.add_data("u", dtype)
        dd.realize()
        assert dd.num_domains() == 1
        self.dd, self.size, self.dtype, self.backend = dd, size, dtype, backend
        self.d = dd.domain(0)
        if layout == "shared_halo_line":
            assert self.d.shared_halo_line()
        self.word = np.uint32 if dtype == torch.float32 else np.uint64
        r = self.d.radius()
        self.r = (r.x(-1), r.y(-1), r.z(-1))
        p = self.d.pitch(self.q)
        self.pitch = (p.x, p.y, p.z)
        self.pad = self.d.pad_x(self.q)
        t = dd.curr(0, self.q)
        rx, ry, rz = self.r
        t[rz:rz + size[2], ry:ry + size[1], rx:rx + size[0]].copy_(global_field(size, dtype).to(t.device))
        self.sync()

    def sync(self):
        if self.backend == _C.Backend.Device:
            torch.cuda.synchronize()

    def rect(self, lo, hi):
        return _C.Rect3(_C.Dim3(*lo), _C.Dim3(*hi))

    def whole(self):
        return ((0, 0, 0), self.size)


_DOMS = {}


def domain(st, backend, size, radius, dtype, layout="padded", fresh=False):
    """domains are reused between the cases that leave curr's interior alone (halos are exchanged again by every
    case); a case that swaps asks for a fresh one. radius: "face1" (group A) or "pair" (face 2, edge 1, corner 0)"""
    key = (backend, size, radius, dtype, layout)
    if fresh or key not in _DOMS:
        rad = st.Radius.face_edge_corner(1, 0, 0) if radius == "face1" else st.Radius.face_edge_corner(2, 1, 0)
        dom = Dom(st, backend, size, rad, dtype, layout)
        if fresh:
            return dom
        _DOMS[key] = dom
    return _DOMS[key]


def drop_domains():
    """free the shared domains (the test modules do at their end, while the runtime is still up)"""
    _DOMS.clear()


def make_tune(st, variant=2, ty=2, nw=8, nontemporal=True, xcd_remap=True, zchunk=0, wrap=0, **more):
    t = st.StencilTune()
    t.variant, t.ty, t.nw, t.nontemporal, t.xcd_remap, t.zchunk, t.wrap = variant, ty, nw, nontemporal, xcd_remap, zchunk, wrap
    for k, v in more.items():
        assert hasattr(t, k), k
        setattr(t, k, v)
    return t


# ---- the check ----
def fill_word(dom):
    """the fill byte repeated over one element: as fp32 / fp64 a finite negative value, which no stencil of values in
    [0, 1) (a mean of non-negative cells, or a sphere's 0 / 1) produces"""
    w = np.frombuffer(bytes([FILL]) * np.dtype(dom.word).itemsize, dtype=dom.word)[0]
    v = float(np.array([w]).view(np.float32 if dom.word == np.uint32 else np.float64)[0])
    assert np.isfinite(v) and v < 0, v
    return w


def prepare(dom, wrap=0):
    """steps 1-3: fill `next`, exchange curr, NaN over the halos of the wrapped axes"""
    fill_word(dom)
    dom.d.fill_bytes(dom.q, FILL, False, True)
    dom.dd.exchange()
    dom.sync()
    if wrap:
        t = dom.dd.curr(0, dom.q)
        for ax, dim in enumerate((2, 1, 0)):  # x, y, z -> tensor dims
            if (wrap >> ax) & 1:
                r, n = dom.r[ax], dom.size[ax]
                t.narrow(dim, 0, r).fill_(float("nan"))
                t.narrow(dim, r + n, t.shape[dim] - r - n).fill_(float("nan"))
        dom.sync()


def check_buffer(dom, regions, ref, what=""):
    """steps 5-7: the whole allocation of `next` against the oracle words `ref` on `regions` ((lo, hi) pairs in
    compute-region coordinates, disjoint) and the fill byte everywhere else"""
    dom.sync()
    raw = dom.d.buffer_to_host(dom.q, False)
    assert len(raw) >= dom.d.buffer_bytes(dom.q) and len(raw) % np.dtype(dom.word).itemsize == 0
    got = np.frombuffer(raw, dtype=dom.word)
    want = np.full_like(got, fill_word(dom))
    inside = np.zeros(got.shape, dtype=bool)
    px, py, _ = dom.pitch
    rx, ry, rz = dom.r
    cells = 0
    for lo, hi in regions:
        if any(b <= a for a, b in zip(lo, hi)):
            continue
        z = np.arange(lo[2], hi[2]).reshape(-1, 1, 1)
        y = np.arange(lo[1], hi[1]).reshape(1, -1, 1)
        x = np.arange(lo[0], hi[0]).reshape(1, 1, -1)
        idx = ((z + rz) * py + (y + ry)) * px + dom.pad + rx + x
        assert not inside[idx].any(), "the case's regions overlap"
        inside[idx] = True
        want[idx] = ref[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        cells += idx.size
    assert int(inside.sum()) == cells
    diff = got != want
    wrong_inside = int((diff & inside).sum())
    wrong_outside = int((diff & ~inside).sum())
    # every other *byte*: a partly overwritten element differs as a word too
    assert wrong_outside == 0, f"{what}: {wrong_outside} elements outside the region(s) were written " \
                               f"(first at element {int(np.flatnonzero(diff & ~inside)[0])}, pitch {dom.pitch}, pad {dom.pad}); " \
                               f"{wrong_inside} of {cells} region cells differ"
    assert wrong_inside == 0, f"{what}: {wrong_inside} of {cells} region cells differ from the oracle " \
                              f"(first at element {int(np.flatnonzero(diff & inside)[0])}); 0 outside"
    assert np.array_equal(got, want)
    return cells


def run_check(dom, call, regions, ref, wrap=0, what=""):
    prepare(dom, wrap)
    call()
    return check_buffer(dom, regions, ref, what)


def check_untouched(dom, what=""):
    return check_buffer(dom, [], None, what)


# =====================================================================================================================
# Group A: the single step
# =====================================================================================================================
# id -> variant, ty, nw, nontemporal, xcd_remap
INSTANCES = {
    "v2-ty2-nw8": (2, 2, 8, True, True),  # the default
    "v0-ty2": (0, 2, 8, True, True), "v0-ty4": (0, 4, 8, True, True), "v0-ty8": (0, 8, 4, True, True),
    "v1-ty4": (1, 4, 8, True, True), "v1-ty8": (1, 8, 8, True, True),
    "v2-ty1": (2, 1, 8, True, True), "v2-nw4": (2, 2, 4, True, True), "v2-nw16": (2, 2, 16, True, True),
    "v3": (3, 2, 8, True, True), "v4": (4, 2, 8, True, True),
    "v0-ty2-plain-stores": (0, 2, 8, False, True), "v0-ty2-no-remap": (0, 2, 8, True, False),
    "v1-ty8-plain-no-remap": (1, 8, 8, False, False),
}
DEFAULT = "v2-ty2-nw8"
MFMA = "mfma"
# one shape per axis group (x remainders, the wave edge, y rows per block, z chunks) for fp64 and Jacobi
GROUP_SHAPES = [((23, 12, 16), 0), ((257, 12, 16), 0), ((24, 17, 16), 0), ((24, 12, 17), 5)]
assert all(s in SHAPES for s in GROUP_SHAPES)
# Jacobi fp32 on the matrix cores: 64x16 tiles
MFMA_SHAPES = [((63, 16, 8), 0), ((64, 16, 8), 0), ((65, 16, 8), 0), ((130, 16, 8), 0), ((64, 15, 8), 0),
               ((64, 17, 8), 0), ((64, 16, 8), 3)]


def instance_tune(st, inst, **kw):
    if inst == MFMA:
        return make_tune(st, variant=8, **kw)  # StencilTune::kMfma
    v, ty, nw, nt, remap = INSTANCES[inst]
    return make_tune(st, variant=v, ty=ty, nw=nw, nontemporal=nt, xcd_remap=remap, **kw)


def single(dom, kind, region, tune):
    lo, hi = region
    return lambda: stencil7_apply(dom.dd, 0, dom.q, dom.rect(lo, hi), kind_of(kind), spheres=kind == "jacobi", tune=tune)


def case_single_shape(st, backend, size, zchunk, inst, kind, dtype, layout="padded"):
    dom = domain(st, backend, size, "face1", dtype, layout)
    tune = instance_tune(st, inst, zchunk=zchunk)
    n = run_check(dom, single(dom, kind, dom.whole(), tune), [dom.whole()], oracle(size, dtype, kind), what=f"{inst} {size}")
    assert n == size[0] * size[1] * size[2]


def case_single_sub_region(st, backend, name, inst, kind, dtype):
    lo, hi = sub_regions(SUB_SIZE)[name]
    dom = domain(st, backend, SUB_SIZE, "face1", dtype)
    tune = instance_tune(st, inst, zchunk=4)
    n = run_check(dom, single(dom, kind, (lo, hi), tune), [(lo, hi)], oracle(SUB_SIZE, dtype, kind), what=f"{inst} {name}")
    assert (n == 0) == (name == "empty")


def case_single_parity(st, backend, inst, kind, dtype, size=(24, 12, 17), zchunk=5):
    """apply, swap, apply: the second call runs on the odd buffer parity, where alternate_z marches every chunk the
    other way; two oracle steps"""
    dom = domain(st, backend, size, "face1", dtype, fresh=True)
    tune = instance_tune(st, inst, zchunk=zchunk)
    assert tune.alternate_z
    call = single(dom, kind, dom.whole(), tune)
    assert dom.d.parity() == 0
    run_check(dom, call, [dom.whole()], oracle(size, dtype, kind, 1), what=f"{inst} even parity")
    dom.dd.swap()
    assert dom.d.parity() == 1
    run_check(dom, call, [dom.whole()], oracle(size, dtype, kind, 2), what=f"{inst} odd parity")


LAYOUT_SIZES = {"unpadded": (21, 9, 7), "shared_halo_line": (96, 12, 9), "align64": (23, 12, 9)}


def case_single_layout(st, backend, layout, inst, kind, dtype, sub=None):
    """unpadded -> stencil7_generic_kernel; shared halo lines at x = 96: the padding behind a row is the next row's -x
    halo (in `next` nothing may land there); the interior on 64-B sectors"""
    size = LAYOUT_SIZES[layout]
    dom = domain(st, backend, size, "face1", dtype, layout)
    if layout == "shared_halo_line":
        assert dom.pad + dom.r[0] + size[0] + 1 > dom.pitch[0], "the +x halo does not reach into the next row's padding"
    region = dom.whole() if sub is None else sub
    tune = instance_tune(st, inst, zchunk=4)
    run_check(dom, single(dom, kind, region, tune), [region], oracle(size, dtype, kind), what=f"{layout} {inst}")


WRAP_CASES = [((24, 12, 9), torch.float32), ((22, 12, 9), torch.float32), ((22, 12, 9), torch.float64)]


def wrap_sub_ranges(size, mask):
    """the whole region, and a sub-range along each axis the mask leaves unwrapped (x sub-ranges start on a 16-B chunk:
    the wrapping kernel's chunk grid starts at the region)"""
    X, Y, Z = size
    out = [((0, 0, 0), size)]
    if not mask & 1:
        out.append(((4, 0, 0), (19, Y, Z)))
    if not mask & 2:
        out.append(((0, 1, 0), (X, Y - 2, Z)))
    if not mask & 4:
        out.append(((0, 0, 2), (X, Y, Z - 1)))
    return out


def case_single_wrap(st, backend, size, dtype, mask, kind):
    dom = domain(st, backend, size, "face1", dtype)
    ok = stencil7_wrappable_axes(dom.dd, 0, dom.q)
    V = 16 // np.dtype(dom.word).itemsize
    assert ok == ((1 if size[0] % V == 0 else 0) | 6), ok
    tune = make_tune(st, wrap=mask, zchunk=4)
    if mask & ~ok:
        prepare(dom, 0)
        with pytest.raises(Exception, match="not supported by this layout"):
            single(dom, kind, dom.whole(), tune)()
        check_untouched(dom, "refused wrap")
        return "refused"
    for region in wrap_sub_ranges(size, mask):
        run_check(dom, single(dom, kind, region, tune), [region], oracle(size, dtype, kind), wrap=mask,
                  what=f"wrap {mask} {region}")
    return "ran"


REGION_SIZE = (37, 13, 11)


def shell_slabs(size, lo_shrink, hi_shrink):
    """the six slabs of the compute region minus the interior shrunk by lo_shrink / hi_shrink (per axis): z slabs are
    whole planes, y slabs span x, x slabs are what is left (as the overlapped steps cut them)"""
    X, Y, Z = size
    ilo = lo_shrink
    ihi = tuple(n - s for n, s in zip(size, hi_shrink))
    slabs = [((0, 0, 0), (X, Y, ilo[2])), ((0, 0, ihi[2]), (X, Y, Z)),
             ((0, 0, ilo[2]), (X, ilo[1], ihi[2])), ((0, ihi[1], ilo[2]), (X, Y, ihi[2])),
             ((0, ilo[1], ilo[2]), (ilo[0], ihi[1], ihi[2])), ((ihi[0], ilo[1], ilo[2]), (X, ihi[1], ihi[2]))]
    return slabs, (ilo, ihi)


def scattered_regions(size, n):
    """n disjoint small regions: one-cell, thin in x (column mode), 8 and more cells wide with unaligned starts"""
    X, Y, Z = size
    out = []
    for k in range(n):
        z = k % Z
        y = (3 * k) % (Y - 2)
        shape = k % 4
        if shape == 0:
            out.append(((1 + k % 5, y, z), (2 + k % 5, y + 1, z + 1)))       # one cell
        elif shape == 1:
            out.append(((9 + k % 3, y, z), (12 + k % 3, y + 2, z + 1)))      # 3 wide: column mode
        elif shape == 2:
            out.append(((14 + k % 3, y, z), (23 + k % 3, y + 1, z + 1)))     # 9 wide, unaligned: row mode
        else:
            out.append(((27, y, z), (X, y + 2, z + 1)))                      # to the +x face
    # no two may share a cell: z differs for k < Z, beyond that the x ranges of equal shape classes repeat 4 apart
    cells = set()
    for lo, hi in out:
        for z in range(lo[2], hi[2]):
            for y in range(lo[1], hi[1]):
                for x in range(lo[0], hi[0]):
                    assert (x, y, z) not in cells, (lo, hi)
                    cells.add((x, y, z))
    return out


def single_region_sets(size):
    X, Y, Z = size
    sets = {f"shell{s}": shell_slabs(size, (s, s, s), (s, s, s))[0] for s in (1, 2, 3)}
    # 7 cells wide = the column mode's widest, 8 = the chunk mode's narrowest; x starts off the chunk grid
    sets["width7and8"] = [((3, 0, 0), (10, Y, 2)), ((13, 0, 0), (21, Y, 2)), ((22, 1, 3), (29, 5, Z)),
                          ((29, 1, 3), (37, 5, Z)), ((1, 6, 3), (9, Y, 5)), ((10, 6, 3), (17, Y, 5))]
    sets["many9"] = scattered_regions(size, 9)
    sets["many17"] = scattered_regions(size, 17)
    return sets


def case_single_regions(st, backend, name, kind, dtype, padded=True):
    """stencil7_apply_regions: padded layout -> stencil7_shell_kernel (row mode for slabs of 8 cells and more in x,
    column mode below), unpadded -> stencil7_regions_kernel; 9 and 17 regions need 2 and 3 tables of 8"""
    size = REGION_SIZE
    dom = domain(st, backend, size, "face1", dtype, "padded" if padded else "unpadded")
    wrap = 0
    if name == "wrap6_x_slabs":
        regions = [((0, 0, 0), (2, size[1], size[2])), ((size[0] - 3, 0, 0), size), ((8, 0, 0), (17, size[1], size[2]))]
        wrap = 6
    else:
        regions = single_region_sets(size)[name]
    tune = make_tune(st, wrap=wrap)
    call = lambda: stencil7_apply_regions(dom.dd, 0, dom.q, [dom.rect(lo, hi) for lo, hi in regions], kind_of(kind),  # noqa: E731
                                          spheres=kind == "jacobi", tune=tune)
    run_check(dom, call, regions, oracle(size, dtype, kind), wrap=wrap, what=f"regions {name}")


def case_single_refusals(st, backend):
    size = (22, 12, 9)
    dom = domain(st, backend, size, "face1", torch.float32)
    prepare(dom, 0)
    device = backend == _C.Backend.Device
    for lo, hi in (((0, 0, 0), (23, 12, 9)), ((-1, 0, 0), (22, 12, 9)), ((0, 0, 0), (22, 12, 10)), ((0, 13, 0), (22, 14, 9))):
        for inst in (DEFAULT, "v1-ty4") + ((MFMA,) if device else ()):
            with pytest.raises(Exception, match="outside compute region"):
                single(dom, "jacobi", (lo, hi), instance_tune(st, inst))()
        if device:
            with pytest.raises(Exception, match="outside compute region"):
                stencil7_apply_regions(dom.dd, 0, dom.q, [dom.rect((0, 0, 0), (1, 1, 1)), dom.rect(lo, hi)],
                                       kind_of("jacobi"), spheres=True)
    if device:
        # a wrapped axis the region does not span
        for mask, region in ((2, ((0, 1, 0), size)), (4, ((0, 0, 0), (22, 12, 8))), (6, ((0, 0, 1), size))):
            with pytest.raises(Exception, match="does not span wrapped axis"):
                single(dom, "astaroth", region, make_tune(st, wrap=mask))()
        # x of 22 fp32 cells is not whole 16-B chunks
        for mask in (1, 3, 5, 7):
            with pytest.raises(Exception, match="not supported by this layout"):
                single(dom, "astaroth", dom.whole(), make_tune(st, wrap=mask))()
            with pytest.raises(Exception, match="not supported by this layout"):
                stencil7_apply_regions(dom.dd, 0, dom.q, [dom.rect(*dom.whole())], kind_of("astaroth"), spheres=False,
                                       tune=make_tune(st, wrap=mask))
        # the MFMA variant: Jacobi only, no in-kernel wrap
        with pytest.raises(Exception, match="Jacobi order"):
            single(dom, "astaroth", dom.whole(), instance_tune(st, MFMA))()
        with pytest.raises(Exception, match="no in-kernel wrap"):
            single(dom, "jacobi", dom.whole(), instance_tune(st, MFMA, wrap=2))()
    else:
        with pytest.raises(Exception, match="in-kernel wrap needs a device sub-domain"):
            stencil7_apply_regions(dom.dd, 0, dom.q, [dom.rect(*dom.whole())], kind_of("astaroth"), spheres=False,
                                   tune=make_tune(st, wrap=2))
    check_untouched(dom, "single-step refusals")


# =====================================================================================================================
# Group B: the fused pair
# =====================================================================================================================
# y around the block's 8 output rows; z as in group A
PAIR_COLUMN_SHAPES = [
    ((20, 9, 8), 0), ((21, 9, 8), 0), ((22, 9, 8), 0), ((23, 9, 8), 0),
    ((255, 9, 6), 0), ((256, 9, 6), 0), ((257, 9, 6), 0), ((513, 9, 6), 0),
    ((24, 7, 8), 0), ((24, 8, 8), 0), ((24, 9, 8), 0), ((24, 17, 8), 0),
    ((24, 9, 7), 0), ((24, 9, 17), 5), ((24, 9, 9), 1), ((24, 9, 40), 0),
]
PAIR_GROUP_SHAPES = [((23, 9, 8), 0), ((257, 9, 6), 0), ((24, 17, 8), 0), ((24, 9, 17), 5)]
PAIR_SCHEDS = [0, 1]  # tune.x2sched: fixed z chunks / the balanced split (an explicit zchunk always gives fixed chunks)
PAIR_SUB_SIZE = SUB_SIZE


def pair_form(dtype, nx, x0, wrap, x2row=1):
    """the form the case expects, from the widths alone (stencil_ops.hpp: X2Form)"""
    es = 4 if dtype == torch.float32 else 8
    V = 16 // es
    if not x2row:
        return "column"
    if es == 4 and (wrap & 1) and x0 % V == 0 and 256 < nx <= 832:
        return "row" if nx == 512 else "ragged2" if nx < 512 else "ragged3" if nx <= 768 else "tail"
    return "col2" if x0 % V == 0 and nx % (128 * V) == 0 else "column"


def pair(dom, kind, region, tune):
    lo, hi = region
    return lambda: stencil7x2_apply(dom.dd, 0, dom.q, dom.rect(lo, hi), kind_of(kind), spheres=kind == "jacobi", tune=tune)


def pair_info(dom, kind, region, tune):
    lo, hi = region
    return stencil7x2_launch_info(dom.dd, 0, dom.q, dom.rect(lo, hi), kind_of(kind), spheres=kind == "jacobi", tune=tune)


def case_pair(st, backend, size, dtype, kind, region=None, form=None, what="", **tune_kw):
    """one fused pair on `region` (default the whole compute region) = two oracle steps; the launch report names the
    expected form (and for an explicit zchunk the fixed-chunk schedule)"""
    dom = domain(st, backend, size, "pair", dtype)
    region = dom.whole() if region is None else region
    tune = make_tune(st, **tune_kw)
    wrap = tune.wrap
    empty = any(b <= a for a, b in zip(*region))
    info = pair_info(dom, kind, region, tune)
    if empty:
        assert info["blocks"] == 0, info
    else:
        want_form = form or pair_form(dtype, region[1][0] - region[0][0], region[0][0], wrap, tune.x2row)
        assert info["form"] == want_form, (info, want_form)
        assert info["wrap_variant"] == (2 if wrap & 1 else 1 if wrap else 0), info
        nz = region[1][2] - region[0][2]
        if tune.zchunk:
            assert info["seg"] == 0 and info["zchunk"] == tune.zchunk and info["gz"] == -(-nz // tune.zchunk), info
        elif tune.x2sched == 0:
            assert info["seg"] == 0 and info["gz"] == -(-nz // info["zchunk"]), info
        else:
            assert info["seg"] >= 1, info
    run_check(dom, pair(dom, kind, region, tune), [region], oracle(size, dtype, kind, 2), wrap=wrap,
              what=f"pair {size} {region} {what} {info}")
    return info


def case_pair_sub_region(st, backend, name, dtype, kind, sched):
    lo, hi = sub_regions(PAIR_SUB_SIZE)[name]
    case_pair(st, backend, PAIR_SUB_SIZE, dtype, kind, region=(lo, hi), form="column", x2sched=sched,
              zchunk=4 if sched == 0 else 0)


def case_pair_parity(st, backend, size, dtype, kind, **tune_kw):
    dom = domain(st, backend, size, "pair", dtype, fresh=True)
    tune = make_tune(st, **tune_kw)
    assert tune.alternate_z
    call = pair(dom, kind, dom.whole(), tune)
    run_check(dom, call, [dom.whole()], oracle(size, dtype, kind, 2), wrap=tune.wrap, what="pair, even parity")
    dom.dd.swap()
    assert dom.d.parity() == 1
    run_check(dom, call, [dom.whole()], oracle(size, dtype, kind, 4), wrap=tune.wrap, what="pair, odd parity")


ROW_WIDTHS = [257, 300, 511, 512, 513, 645, 768, 769, 813, 832]
ROW_FORMS = {257: "ragged2", 300: "ragged2", 511: "ragged2", 512: "row", 513: "ragged3", 645: "ragged3", 768: "ragged3",
             769: "tail", 813: "tail", 832: "tail"}


def pair_row_cases():
    """(width, y, z, wrap, x2early, sub): every width at y in {7, 9} x z in {5, 17} with wrap 1, 3, 5 and 7; x2early
    off and the y / z sub-ranges (wrap 1: y and z are read from halos) at (9, 17)"""
    out = []
    for nx in ROW_WIDTHS:
        for y in (7, 9):
            for z in (5, 17):
                for wrap in (1, 3, 5, 7):
                    out.append((nx, y, z, wrap, True, None))
        for wrap in (1, 7):
            out.append((nx, 9, 17, wrap, False, None))
        out.append((nx, 9, 17, 1, True, "y"))
        out.append((nx, 9, 17, 1, True, "z"))
        out.append((nx, 9, 17, 1, False, "yz"))
    return out


def row_case_id(c):
    nx, y, z, wrap, early, sub = c
    return f"{nx}x{y}x{z}-wrap{wrap}" + ("" if early else "-late") + (f"-sub{sub}" if sub else "")


def case_pair_row(st, backend, c):
    nx, y, z, wrap, early, sub = c
    size = (nx, y, z)
    lo, hi = [0, 0, 0], [nx, y, z]
    if sub and "y" in sub:
        lo[1], hi[1] = 1, y - 2
    if sub and "z" in sub:
        lo[2], hi[2] = 2, z - 3
    kind = "jacobi" if (y, z) == (9, 17) else "astaroth"
    dom = domain(st, backend, size, "pair", torch.float32)
    assert stencil7x2_wrappable_axes(dom.dd, 0, dom.q) == 7
    case_pair(st, backend, size, torch.float32, kind, region=(tuple(lo), tuple(hi)), form=ROW_FORMS[nx], wrap=wrap,
              x2early=early)


# (size, dtype, region or None, wrap)
PAIR_COL2_CASES = [
    ((512, 9, 5), torch.float32, None, 0), ((1024, 9, 5), torch.float32, None, 0), ((256, 9, 5), torch.float64, None, 0),
    # starts on a chunk and is 512 wide, but is no memory-aligned column
    ((1040, 9, 5), torch.float32, ((4, 0, 0), (516, 9, 5)), 0),
    ((512, 9, 9), torch.float32, ((0, 0, 2), (512, 9, 7)), 2), ((512, 9, 9), torch.float32, None, 2),
    ((512, 9, 9), torch.float32, ((0, 1, 0), (512, 8, 9)), 4), ((512, 9, 9), torch.float32, None, 4),
    ((1024, 9, 5), torch.float32, ((512, 0, 0), (1024, 9, 5)), 6), ((1024, 9, 5), torch.float32, None, 6),
    ((256, 9, 5), torch.float64, None, 6),
]


def col2_case_id(c):
    size, dtype, region, wrap = c
    return f"{size[0]}x{size[1]}x{size[2]}-{dtype_id(dtype)}-wrap{wrap}" + ("-sub" if region else "")


def case_pair_col2(st, backend, c, kind, early=True, xfast=0):
    size, dtype, region, wrap = c
    case_pair(st, backend, size, dtype, kind, region=region, form="col2", wrap=wrap, x2early=early, x2xfast=xfast)


EXTERIOR_CASES = [((40, 21, 19), torch.float32), ((38, 21, 19), torch.float64)]
# lo shrink, hi shrink per axis: equal 1-5 (thickest slab <= 2 and 3-4: the two thin-kernel instances; 5: one thread per
# cell), unequal with empty slabs
EXTERIOR_WRAPS = {1: ((0, 2, 1), (0, 1, 3)), 2: ((2, 0, 1), (3, 0, 2)), 4: ((1, 2, 0), (2, 3, 0))}
EXTERIOR_SHRINKS = {
    "s1": ((1, 1, 1), (1, 1, 1)), "s2": ((2, 2, 2), (2, 2, 2)), "s3": ((3, 3, 3), (3, 3, 3)), "s4": ((4, 4, 4), (4, 4, 4)),
    "s5": ((5, 5, 5), (5, 5, 5)),
    "unequal_thin": ((0, 2, 1), (2, 0, 1)), "unequal": ((1, 0, 4), (3, 2, 0)), "unequal_thick": ((0, 6, 1), (2, 0, 0)),
    "x_only": ((2, 0, 0), (3, 0, 0)), "z_only": ((0, 0, 2), (0, 0, 1)),
}


def case_pair_exterior(st, backend, size, dtype, kind, shrink, wrap=0):
    """the exterior alone: shell cells = two oracle steps, interior cells keep the fill; then the interior sweep on top
    of it: every compute cell written and nothing else"""
    lo_s, hi_s = EXTERIOR_SHRINKS[shrink] if isinstance(shrink, str) else shrink
    dom = domain(st, backend, size, "pair", dtype)
    slabs, (ilo, ihi) = shell_slabs(size, lo_s, hi_s)
    for ax in range(3):
        assert not (wrap >> ax) & 1 or (lo_s[ax] == 0 and hi_s[ax] == 0), "the interior spans a wrapped axis"
    tune = make_tune(st, wrap=wrap)
    ref = oracle(size, dtype, kind, 2)
    call = lambda: stencil7x2_apply_exterior(dom.dd, 0, dom.q, dom.rect(ilo, ihi), kind_of(kind),  # noqa: E731
                                             spheres=kind == "jacobi", tune=tune)
    n = run_check(dom, call, slabs, ref, wrap=wrap, what=f"exterior {shrink} wrap {wrap}")
    assert n == size[0] * size[1] * size[2] - (ihi[0] - ilo[0]) * (ihi[1] - ilo[1]) * (ihi[2] - ilo[2])
    pair(dom, kind, (ilo, ihi), tune)()
    check_buffer(dom, [dom.whole()], ref, what=f"exterior {shrink} wrap {wrap} + interior")


def case_pair_regions(st, backend, n, dtype, kind, wrap):
    size = REGION_SIZE
    dom = domain(st, backend, size, "pair", dtype)
    regions = scattered_regions(size, n)
    call = lambda: stencil7x2_apply_regions(dom.dd, 0, dom.q, [dom.rect(lo, hi) for lo, hi in regions], kind_of(kind),  # noqa: E731
                                            spheres=kind == "jacobi", wrap=wrap)
    run_check(dom, call, regions, oracle(size, dtype, kind, 2), wrap=wrap, what=f"pair regions {n} wrap {wrap}")


def case_pair_refusals(st, backend):
    size = (22, 12, 9)
    dom = domain(st, backend, size, "pair", torch.float32)
    prepare(dom, 0)
    K = kind_of("astaroth")
    for lo, hi in (((0, 0, 0), (23, 12, 9)), ((-1, 0, 0), (22, 12, 9)), ((0, 0, 0), (22, 12, 10)), ((0, 13, 0), (22, 14, 9))):
        with pytest.raises(Exception, match="outside compute region"):
            pair(dom, "astaroth", (lo, hi), make_tune(st))()
        with pytest.raises(Exception, match="outside compute region"):
            pair_info(dom, "astaroth", (lo, hi), make_tune(st))
        with pytest.raises(Exception, match="outside compute region"):
            stencil7x2_apply_regions(dom.dd, 0, dom.q, [dom.rect((0, 0, 0), (1, 1, 1)), dom.rect(lo, hi)], K, spheres=False)
        with pytest.raises(Exception, match="outside compute region"):
            stencil7x2_apply_exterior(dom.dd, 0, dom.q, dom.rect(lo, hi), K, spheres=False)
    for mask, region in ((2, ((0, 1, 0), size)), (4, ((0, 0, 0), (22, 12, 8))), (6, ((0, 0, 1), size))):
        with pytest.raises(Exception, match="does not span wrapped axis"):
            pair(dom, "astaroth", region, make_tune(st, wrap=mask))()
        with pytest.raises(Exception, match="does not span wrapped axis"):
            stencil7x2_apply_exterior(dom.dd, 0, dom.q, dom.rect(*region), K, spheres=False, tune=make_tune(st, wrap=mask))
    # 22 fp32 cells are not whole chunks, and no row form takes rows this short
    assert stencil7x2_wrappable_axes(dom.dd, 0, dom.q) == 6
    for mask in (1, 3, 5, 7):
        with pytest.raises(Exception, match="not supported by this layout"):
            pair(dom, "astaroth", dom.whole(), make_tune(st, wrap=mask))()
    check_untouched(dom, "pair refusals")
    # ragged rows the whole-row kernel would wrap, with that kernel switched off
    dom = domain(st, backend, (301, 9, 5), "pair", torch.float32)
    prepare(dom, 0)
    assert stencil7x2_wrappable_axes(dom.dd, 0, dom.q, 1) == 7 and stencil7x2_wrappable_axes(dom.dd, 0, dom.q, 0) == 6
    with pytest.raises(Exception, match="not supported by this layout"):
        pair(dom, "astaroth", dom.whole(), make_tune(st, wrap=1, x2row=0))()
    check_untouched(dom, "pair refusals, x2row 0")
