"""The fused pairs' kernel form and block schedule (stencil_ops.hpp stencil7x2_form / stencil7x2_schedule), the one
decision stencil7x2_apply, stencil7x2_launch_info, stencil7x2_row_kernel_used and stencil7x2_wrappable_axes share.
Expected values are the documented ones (README design notes, the x2_lockstep_schedule comment, the docstrings of
tests/test_gpu.py::test_temporal2_*), not read back from the code. CPU only (pure host functions); the GPU side is
tests/test_gpu.py::test_temporal2_*."""
import pytest

from stencil2_amd import _C

BIG = (1 << 32) - 4096  # the row forms address the field by 32-bit buffer offsets


def _tune(**kw):
    t = _C.StencilTune()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("nx,form", [(512, "row"), (257, "ragged2"), (511, "ragged2"), (513, "ragged3"),
                                     (645, "ragged3"), (768, "ragged3"), (769, "tail"), (813, "tail"), (832, "tail"),
                                     (1024, "col2"), (2048, "col2"), (256, "column"), (836, "column")])
def test_form_fp32_periodic_rows(nx, form):
    """fp32, x wrapped in-kernel, the region on a chunk, a field under 4 GiB"""
    assert _C.stencil7x2_form(4, nx, x0=0, wrap=1, x2row=1, buffer_bytes=nx * 64 * 64 * 4) == form
    assert _C.stencil7x2_form(4, nx, x0=8, wrap=7, x2row=1) == form


@pytest.mark.parametrize("kw,form", [
    # x from halos: no row form
    (dict(elem_size=4, nx=512, wrap=0), "col2"), (dict(elem_size=4, nx=1024, wrap=6), "col2"),
    (dict(elem_size=4, nx=645, wrap=6), "column"),
    # a first cell off the 16-B chunk grid
    (dict(elem_size=4, nx=512, x0=1), "column"), (dict(elem_size=4, nx=645, x0=2), "column"),
    (dict(elem_size=4, nx=813, x0=3), "column"), (dict(elem_size=4, nx=1024, x0=5), "column"),
    # x2row = 0: always the one-chunk column kernel
    (dict(elem_size=4, nx=512, x2row=0), "column"), (dict(elem_size=4, nx=645, x2row=0), "column"),
    (dict(elem_size=4, nx=1024, x2row=0), "column"), (dict(elem_size=8, nx=256, x2row=0), "column"),
    # fields of 4 GiB - 4096 bytes or more: the row forms refuse, whole two-chunk columns still run col2
    (dict(elem_size=4, nx=512, buffer_bytes=BIG), "col2"), (dict(elem_size=4, nx=645, buffer_bytes=BIG), "column"),
    (dict(elem_size=4, nx=512, buffer_bytes=BIG - 1), "row"),
    # fp64: 256-cell columns (two 2-double chunks per lane), never a row form
    (dict(elem_size=8, nx=256), "col2"), (dict(elem_size=8, nx=1024), "col2"), (dict(elem_size=8, nx=1024, wrap=0), "col2"),
    (dict(elem_size=8, nx=300), "column"), (dict(elem_size=8, nx=512, buffer_bytes=BIG), "col2"),
    (dict(elem_size=8, nx=256, x0=1), "column"), (dict(elem_size=8, nx=256, x0=2), "col2"),
    # boundary-plane publication: only the row forms publish (anything else is the fallback, which apply refuses)
    (dict(elem_size=4, nx=512, publishing=True), "row"), (dict(elem_size=4, nx=813, publishing=True), "tail"),
    (dict(elem_size=4, nx=1024, publishing=True), "column"), (dict(elem_size=8, nx=256, publishing=True), "column"),
])
def test_form_other_conditions(kw, form):
    assert _C.stencil7x2_form(**kw) == form


def _sched(form, cols, nz, slots=256, resident=256, **kw):
    return _C.stencil7x2_schedule(form, cols, nz, resident, slots, _tune(**kw))


@pytest.mark.parametrize("cols,nz,seg,parts,blocks,rounds", [
    (40, 112, 2, 6, 240, 1),   # 40 columns: P = 6 over 240 blocks
    (25, 160, 2, 10, 250, 1),  # 25 ragged 645-cell columns: P = 10
    (17, 256, 2, 15, 255, 1),  # 17 tail-row columns: P = 15 over 255
    (70, 112, 3, 7, 245, 2),   # 70 row groups: 2 rounds x 35 groups x 7 parts
    (81, 240, 2, 4, 256, 1),   # 81 row groups: quarters over 64 + 17 leftover groups as second segments
    (264, 16, 3, 1, 132, 2),   # more row groups than blocks: 2 rounds of whole columns
])
def test_schedule_row_forms_lockstep(cols, nz, seg, parts, blocks, rounds):
    for form in ("row", "ragged2", "ragged3", "tail"):
        s = _sched(form, cols, nz)
        assert (s["seg"], s["parts"], s["blocks"], s["rounds"]) == (seg, parts, blocks, rounds), (form, s)
        assert (s["parts"], s["blocks"], s["rounds"]) == _C.x2_lockstep_schedule(256, cols, nz)


def test_schedule_balanced_split():
    """parts under 16 planes: no lockstep, one block per slot but pieces of at least 16 planes"""
    s = _sched("row", 15, 116)  # 17 parts would be 6 planes each
    assert (s["seg"], s["parts"], s["rounds"], s["blocks"]) == (1, 0, 1, 108)  # min(256, 15 * 116 // 16)
    s = _sched("row", 40, 112, x2lockstep=False)
    assert (s["seg"], s["parts"], s["blocks"]) == (1, 0, 256)
    assert _sched("row", 1, 8)["blocks"] == 1


def test_schedule_two_chunk_columns():
    """the 512-cell column kernel over 2 x 16 columns: P = 8; lockstep only with the columns y-major (x2xfast = 0);
    4 x 130 columns: 3 rounds"""
    s = _sched("col2", 32, 128)
    assert (s["seg"], s["parts"], s["blocks"], s["rounds"]) == (2, 8, 256, 1)
    s = _sched("col2", 32, 128, x2xfast=1)
    assert (s["seg"], s["parts"], s["blocks"]) == (1, 0, 256)
    s = _sched("col2", 520, 16)
    assert (s["seg"], s["parts"], s["blocks"], s["rounds"]) == (3, 1, 174, 3)


@pytest.mark.parametrize("cols,nz", [(40, 112), (25, 160), (17, 256), (70, 112), (81, 240), (264, 16), (520, 16),
                                     (15, 116), (1, 64)])
def test_schedule_column_form_never_runs_lockstep(cols, nz):
    s = _sched("column", cols, nz)
    assert (s["seg"], s["parts"], s["rounds"]) == (1, 0, 1)
    assert s["blocks"] == max(1, min(256, cols * nz // 16))


@pytest.mark.parametrize("form", ["row", "ragged3", "col2", "column"])
@pytest.mark.parametrize("cols,nz", [(40, 112), (64, 4), (7, 2), (264, 16), (86, 512)])
def test_schedule_fixed_z_chunks(form, cols, nz):
    """x2sched = 0 or a given zchunk: blocks of fixed z chunks per column (the exterior's z slabs run one chunk = the
    slab), no segments"""
    for kw in (dict(x2sched=0), dict(zchunk=5), dict(x2sched=0, zchunk=nz), dict(zchunk=1000)):
        s = _sched(form, cols, nz, **kw)
        zc = s["zchunk"]
        assert s["seg"] == 0 and s["parts"] == 0 and s["rounds"] == 1
        assert zc >= 1 and s["gz"] == -(-nz // zc) and s["blocks"] == cols * s["gz"]
        if "zchunk" in kw:
            assert zc == kw["zchunk"]


def test_slots_leave_the_reserved_cus_free():
    """one block per CU on 256 CUs: 8 CUs left to the transports leave 248 slots; never more than half the CUs, never
    fewer slots than the blocks of one CU"""
    assert _C.slots_less_reserved(256, 8, 256) == 248
    assert _C.slots_less_reserved(256, 0, 256) == 256
    assert _C.slots_less_reserved(512, 8, 256) == 496
    assert _C.slots_less_reserved(256, 200, 256) == 128
    assert _C.slots_less_reserved(1, 8, 256) == 1
    # and the schedule then runs on those slots: 512^3's 64 row groups on 248 blocks march quarters
    s = _sched("row", 64, 512, slots=248)
    assert (s["seg"], s["parts"], s["blocks"]) == (2, 4, 248)
