"""Cases shared by test_copy_types.py (host backend, memmove path) and test_gpu_copy_types.py (the HIP copy kernel):
byte-exact region copies steered into every (vector width, row width) instance of the copy kernel, work-table edges,
and exchanges of nine quantities of mixed element sizes against the byte oracle of stencil2_amd.utils.testing."""
import contextlib

import numpy as np
import torch

from stencil2_amd import _C
from stencil2_amd.parallel.domain import _TORCH_TO_DT
from stencil2_amd.utils.testing import check_exchange_bytes, fill_bytes_pattern

POISON = 0xFF

# ---- region copies ----
REGION_SIZE, REGION_RADIUS = (37, 9, 7), 2
REGION_ES = [1, 2, 3, 4, 6, 8, 12, 16]
REGION_PX = list(range(6))
REGION_EX = list(range(1, 10)) + [16, 17, 33]
VECS = (16, 8, 4, 2, 1)
WIDTHS = (1, 2, 3, 4, 5)  # row widths 1..4 units (one row per item) and 5 = wide (one unit per item)


def region_domain(st, backend, size=REGION_SIZE, radius=REGION_RADIUS, sizes=REGION_ES):
    """one sub-domain holding an opaque quantity per element size; returns (dd, local domain, {es: quantity})"""
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius)
    dd.set_gpus([0])
    qs = {es: dd.native.add_data(es, f"b{es}") for es in sizes}
    dd.realize()
    assert dd.num_domains() == 1
    return dd, dd.domain(0), qs


def region_shape(d, q, pos, ext):
    """(vec, min(row_units, 5)) of the kernel instance a region copy of this box runs: make_copy_seg on the real
    addresses. The dense side has base 0: device and host allocations are at least 256-B aligned."""
    es = d.elem_size(q)
    p = d.pitch(q)
    ys, zs = p.x * es, p.x * p.y * es
    ptr = d.curr_ptr(q) + pos[0] * es + pos[1] * ys + pos[2] * zs
    s = _C.copy_seg_shape(0, ext[0] * es, ext[0] * ext[1] * es, ptr, ys, zs, _C.Dim3(*ext), es)
    assert s["ny"] == ext[1] and s["units"] == s["row_units"] * ext[1] * ext[2] and s["vec"] * s["row_units"] == ext[0] * es
    assert s["rows"] == (s["row_units"] <= 4)  # region copies never carry the whole-sector flag
    # the reverse copy (region_to_host) has the same shape
    assert s == _C.copy_seg_shape(ptr, ys, zs, 0, ext[0] * es, ext[0] * ext[1] * es, _C.Dim3(*ext), es)
    return s["vec"], min(s["row_units"], 5)


def check_region(d, q, pos, ext, rng):
    """poison, write random bytes into the box, read the whole raw allocation back: the box holds the data, every
    other byte is still poison, and region_to_host of the box returns the data (all bitwise)"""
    es = d.elem_size(q)
    raw = d.raw_size()
    d.fill_bytes(q, POISON, True, False)
    data = rng.integers(0, 256, size=(ext[2], ext[1], ext[0], es), dtype=np.uint8)
    P, E = _C.Dim3(*pos), _C.Dim3(*ext)
    d.region_from_host(P, E, q, data.tobytes(), True)
    got = np.frombuffer(d.quantity_to_host(q), dtype=np.uint8).reshape(raw.z, raw.y, raw.x, es)
    want = np.full_like(got, POISON)
    want[pos[2]:pos[2] + ext[2], pos[1]:pos[1] + ext[1], pos[0]:pos[0] + ext[0]] = data
    where = f"es {es} pos {pos} ext {ext}"
    box = got[pos[2]:pos[2] + ext[2], pos[1]:pos[1] + ext[1], pos[0]:pos[0] + ext[0]]
    assert np.array_equal(box, data), f"{where}: {int((box != data).any(axis=-1).sum())} cells of the box are wrong"
    assert np.array_equal(got, want), f"{where}: {int((got != want).sum())} bytes outside the box were written"
    back = np.frombuffer(d.region_to_host(P, E, q, True), dtype=np.uint8).reshape(data.shape)
    assert np.array_equal(back, data), f"{where}: region_to_host returned {int((back != data).any(axis=-1).sum())} wrong cells"


def sweep_boxes():
    return [((px, 2, 1), (ex, 5, 4)) for px in REGION_PX for ex in REGION_EX]


def case_region_sweep(st, backend, es):
    _, d, qs = region_domain(st, backend)
    rng = np.random.default_rng(1000 + es)
    for pos, ext in sweep_boxes():
        check_region(d, qs[es], pos, ext, rng)


def case_region_coverage(st, backend):
    """the sweep runs all 25 (vec, row width) instances of the copy kernel"""
    _, d, qs = region_domain(st, backend)
    seen = {}
    for es, q in qs.items():
        for pos, ext in sweep_boxes():
            seen.setdefault(region_shape(d, q, pos, ext), (es, pos, ext))
    missing = sorted({(v, w) for v in VECS for w in WIDTHS} - set(seen))
    assert not missing, f"(vec, row width) instances the sweep never runs: {missing}"
    assert len(seen) == 25, sorted(seen)
    # the examples every reader can check by hand
    assert region_shape(d, qs[4], (2, 2, 1), (12, 5, 4)) == (16, 3)  # the interior starts on a 128-B line
    assert region_shape(d, qs[6], (0, 2, 1), (1, 5, 4)) == (2, 3)
    assert region_shape(d, qs[3], (0, 2, 1), (1, 5, 4)) == (1, 3)
    return seen


@contextlib.contextmanager
def copy_settings(block_items=None, small_rows=None):
    """global work-table settings for the plans built inside; the defaults come back whatever happens"""
    try:
        if block_items:
            _C.set_copy_block_items(*block_items)
        if small_rows:
            _C.set_copy_small_rows(*small_rows)
        yield
    finally:
        _C.set_copy_block_items(1024, 512)
        _C.set_copy_small_rows(4096, 64)


# one box per row width for each of the two element sizes (region_shape asserts the widths), plus odd offsets
SMALL_ENTRY_BOXES = {
    4: [((2, 2, 1), (4, 5, 4), (16, 1)), ((1, 2, 1), (2, 5, 4), (4, 2)), ((3, 2, 1), (3, 5, 4), (4, 3)),
        ((2, 2, 1), (16, 5, 4), (16, 4)), ((1, 2, 1), (17, 5, 4), (4, 5)), ((0, 2, 1), (33, 5, 4), (4, 5)),
        ((2, 2, 1), (8, 5, 4), (16, 2)), ((5, 2, 1), (1, 5, 4), (4, 1))],
    1: [((0, 2, 1), (1, 5, 4), (1, 1)), ((1, 2, 1), (2, 5, 4), (1, 2)), ((4, 2, 1), (3, 5, 4), (1, 3)),
        ((3, 2, 1), (4, 5, 4), (1, 4)), ((5, 2, 1), (9, 5, 4), (1, 5)), ((2, 2, 1), (16, 5, 4), (16, 1)),
        ((0, 2, 1), (6, 5, 4), (2, 3)), ((2, 2, 1), (33, 5, 4), (1, 5))],
}


def case_small_entries(st, backend, es):
    """5 rows / 7 units per work-table entry and 3-row entries for segments of at most 4 rows: every copy is many
    entries, with partial last entries of both kinds (20 rows = 4 entries of 5; 4-row boxes = 3 + 1; wide boxes end in
    a partial 7-unit entry)"""
    _, d, qs = region_domain(st, backend, sizes=[es])
    rng = np.random.default_rng(2000 + es)
    with copy_settings((5, 7), (4, 3)):
        for pos, ext, shape in SMALL_ENTRY_BOXES[es]:
            assert region_shape(d, qs[es], pos, ext) == shape, (pos, ext)
            check_region(d, qs[es], pos, ext, rng)
        # a segment of at most 4 rows: entries of 3 rows and 1 row
        check_region(d, qs[es], (1, 3, 2), (3, 2, 2), rng)
        check_region(d, qs[es], (1, 3, 2), (2, 4, 1), rng)


def case_default_entries(st, backend, es, ext, rows):
    """narrow rows at the default settings in a (6, 72, 62) radius-1 domain: ext (2, 70, 60) is 4200 rows (1024-row
    entries, four items per thread, the last entry holds 104), ext (2, 60, 60) is 3600 rows (64-row entries of a small
    segment, the last holds 16)"""
    _, d, qs = region_domain(st, backend, size=(6, 72, 62), radius=1, sizes=[es])
    assert ext[1] * ext[2] == rows
    with copy_settings():
        for pos in ((1, 1, 1), (2, 2, 2)):
            assert region_shape(d, qs[es], pos, ext)[1] <= 4
            check_region(d, qs[es], pos, ext, np.random.default_rng(rows + es))


def case_wide_four_items(st, backend, es):
    """1024 units per wide entry: a box of 33 x 9 x 5 cells is 1485 units at vec = es (more than 1024, no multiple of
    256), so threads carry four wide items and the last entry (461 units) ends in a partial tail"""
    _, d, qs = region_domain(st, backend, sizes=[es])
    pos, ext = (3, 0, 1), (33, 9, 5)
    with copy_settings((1024, 1024)):
        assert region_shape(d, qs[es], pos, ext) == (es, 5)
        check_region(d, qs[es], pos, ext, np.random.default_rng(3000 + es))


# ---- exchanges of mixed element types ----
# in this order, so that neighbouring segments of one plan differ in vec
MIXED = [("u8", torch.uint8), ("f16", torch.float16), ("b3", 3), ("f32", torch.float32), ("b6", 6), ("i64", torch.int64),
         ("b12", 12), ("b16", 16), ("b24", 24)]


# the element sizes that divide a 128-B line: a domain of these alone takes the shared-halo-line layout
LINE_TYPES = [m for m in MIXED if m[0] in ("u8", "f16", "f32", "i64", "b16")]


def add_mixed(dd, types=MIXED):
    qs = []
    for name, t in types:
        qs.append(dd.add_data(name, t) if isinstance(t, torch.dtype) else dd.native.add_data(t, name))
    assert qs == list(range(len(types)))
    return qs


def radii(st):
    a = st.Radius.constant(0)
    a.set_dir(1, 0, 0, 2)
    a.set_dir(-1, 0, 0, 1)
    return {"r1": st.Radius.constant(1), "r3": st.Radius.constant(3), "asym": a,
            "fec": st.Radius.face_edge_corner(2, 1, 1)}


def transport_for(st, method):
    """(TransportOptions, MethodFlags) of a method name; PeerCopyEngine = PeerCopy through packed DMA-engine pipes"""
    tr = st.TransportOptions()
    if method == "PeerCopyEngine":
        tr.peer_copy = st.TransportOptions.Copy.Engine
        method = "PeerCopy"
    return tr, getattr(st.MethodFlags, method)


def mixed_domain(st, backend, size, radius, gpus, method, layout=None, types=MIXED):
    tr, flags = transport_for(st, method)
    if layout == "x_face_sectors":
        tr.x_face_sectors = True
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_transport_options(tr)
    dd.set_radius(radius)
    dd.set_gpus(gpus)
    dd.set_methods(flags)
    if layout == "shared_halo_line":
        dd.set_shared_halo_line(True)
    elif layout == "x_halo_align":
        dd.set_x_halo_align(True)
    qs = add_mixed(dd, types)
    dd.realize()
    assert dd.num_domains() == len(gpus)
    return dd, qs


def exchange_twice(dd, qs, radius):
    for tag in (0, 1):
        for q in qs:
            fill_bytes_pattern(dd, q, tag)
        dd.exchange()
        bad = {dd.domain(0).name(q): check_exchange_bytes(dd, q, radius, tag) for q in qs}
        assert not any(bad.values()), f"tag {tag}: wrong cells per quantity {bad}"
        dd.swap()


def case_exchange(st, backend, method, gpus, rname):
    radius = radii(st)[rname]
    dd, qs = mixed_domain(st, backend, (19, 13, 11), radius, gpus, method)
    exchange_twice(dd, qs, radius)


LAYOUTS = ["shared_halo_line", "x_halo_align", "x_face_sectors"]
LAYOUT_DOMAINS = [((128, 13, 11), [0]), ((256, 13, 11), [0, 0])]


def case_layout(st, backend, layout, size, gpus, rname):
    """Some quantities take the special layout and others the plain fallback in the same domain: the halo-aligned x
    layout and the whole-line x faces are chosen per quantity (element sizes that divide 16 B / a 128-B line). Shared
    halo lines are all or nothing, and sizes 3, 6, 12 and 24 switch them off for the whole domain (the request then
    has to leave the plain layout exact; case_shared_lines_active runs the layout itself)."""
    radius = radii(st)[rname]
    dd, qs = mixed_domain(st, backend, size, radius, gpus, "Kernel", layout=layout)
    for d in (dd.domain(i) for i in range(dd.num_domains())):
        if layout == "shared_halo_line":
            assert not d.shared_halo_line()
        for q in qs:
            es, rxm = d.elem_size(q), d.radius().x(-1)
            if 128 % es:  # no padded layout at all: rows of raw cells back to back
                assert d.pad_x(q) == 0 and d.pitch(q).x == d.raw_size().x
            elif layout == "x_halo_align" and 16 % es == 0:
                assert d.pad_x(q) * es < 16 and (d.pad_x(q) + rxm) * es % 16 == 0
            else:
                assert (d.pad_x(q) + rxm) * es % 128 == 0 and d.pitch(q).x * es % 128 == 0
    exchange_twice(dd, qs, radius)


def case_shared_lines_active(st, backend, size, gpus, rname):
    """Only element sizes that divide a line: the shared-halo-line layout is really on, with 1- and 2-byte elements
    among the paired x-face rows."""
    radius = radii(st)[rname]
    dd, qs = mixed_domain(st, backend, size, radius, gpus, "Kernel", layout="shared_halo_line", types=LINE_TYPES)
    assert all(dd.domain(i).shared_halo_line() for i in range(dd.num_domains()))
    exchange_twice(dd, qs, radius)


def case_typed_views(st, backend):
    """DLPack pitch and strides of every named dtype, 1- and 2-byte elements included: after an exchange the torch
    view of the whole allocation holds exactly the bytes quantity_to_host returns"""
    radius = radii(st)["fec"]
    dd = st.DistributedDomain(19, 13, 11, group=st.make_single_group())
    dd.set_backend(backend)
    dd.set_radius(radius)
    dd.set_gpus([0, 0])
    qs = {dd.add_data(str(t).split(".")[-1], t): t for t in _TORCH_TO_DT}
    assert len(qs) == 8
    dd.realize()
    for q in qs:
        fill_bytes_pattern(dd, q, 3)
    dd.exchange()
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    for q, t in qs.items():
        assert check_exchange_bytes(dd, q, radius, 3) == 0, t
        for di in range(dd.num_domains()):
            d = dd.domain(di)
            raw, es = d.raw_size(), d.elem_size(q)
            view = dd.curr(di, q)
            assert view.dtype == t and tuple(view.shape) == (raw.z, raw.y, raw.x) and view.element_size() == es
            p = d.pitch(q)
            assert view.stride() == (p.x * p.y, p.x, 1) and view.data_ptr() == d.curr_ptr(q)
            got = view.cpu().contiguous().view(ints[es]).numpy().view(np.uint8).reshape(raw.z, raw.y, raw.x, es)
            want = np.frombuffer(d.quantity_to_host(q), dtype=np.uint8).reshape(got.shape)
            assert np.array_equal(got, want), f"{t} domain {di}: {int((got != want).any(axis=-1).sum())} cells differ"
