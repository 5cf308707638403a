"""Fused triples where a sub-domain has more (row group, column) pairs than resident blocks, or an even group count
that two lockstep rounds fill (the lockstep rounds schedule, StencilArgs::seg == 3). Rounds exist only in
stencil7x3_xh_kernel; stencil7x3_wrap_kernel (whole 512-cell fp32 rows) has no round loop, so the host schedule
(_C.stencil7x3_schedule) must never hand it rounds: it runs lockstep parts plus second segments, or the balanced split.
A whole-row sweep that did get rounds would launch and write nothing.

Every case first asserts, through ops.stencil7x3_launch_info, the schedule it runs on (the figures hold for 256
resident blocks, one MI355X; on another device the assertion fails with the reported numbers), then compares bitwise
with the torch oracle. Sizes are (x, y, z); y = 1539 and y = 771 are no multiple of the block's 6 output rows, so the
last row group has rows past the y end."""
import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (astaroth_step_reference, jacobi_step_reference, stencil7x3_apply, stencil7x3_launch_info,
                              stencil7x3_supported)

pytestmark = pytest.mark.gpu

# form, kind, fp64, size, x3sched, wrap_self, model wrap axes, ragged, run lengths, (rounds, parts, blocks): for the XH
# form what the launch must be; for the whole-row form what the XH schedule gives for the same (cols, nz, slots), i.e.
# the rounds the whole-row launch must NOT be on
CASES = [
    ("wrap", "astaroth", False, (512, 1539, 16), 1, True, 7, False, (3, 7, 2), (2, 1, 129)),
    ("wrap", "astaroth", False, (512, 1539, 32), 1, True, 7, False, (3, 7, 2), (3, 2, 172)),
    ("wrap", "jacobi", False, (512, 1539, 112), 1, True, 7, False, (3, 4), (5, 4, 208)),
    ("wrap", "astaroth", False, (512, 610, 80), 0, True, 7, False, (3, 7, 2), (2, 5, 255)),
    ("wrap", "astaroth", False, (512, 1539, 16), 0, True, 7, False, (3, 7, 2), (2, 1, 129)),
    ("xh", "astaroth", False, (1024, 771, 16), 1, False, 0, False, (3, 7, 2), (2, 1, 129)),
    ("xh", "astaroth", False, (1024, 771, 32), 1, False, 0, False, (3, 7, 2), (3, 2, 172)),  # last round partly filled
    ("xh", "astaroth", False, (1024, 304, 80), 0, False, 0, False, (3, 7, 2), (2, 5, 255)),
    ("xh", "astaroth", True, (256, 1539, 16), 1, True, 6, False, (3, 7, 2), (2, 1, 129)),
    ("xh", "astaroth", True, (512, 771, 32), 1, True, 6, False, (3, 7, 2), (3, 2, 172)),
    ("xh", "jacobi", True, (512, 771, 112), 1, True, 6, False, (3, 4), (5, 4, 208)),
    ("xh", "astaroth", False, (645, 771, 32), 1, False, 0, True, (3, 7, 2), (3, 2, 172)),  # second column partial
    ("xh", "astaroth", True, (300, 771, 16), 1, False, 0, True, (3, 7, 2), (2, 1, 129)),
]


def _id(c):
    return f"{c[0]}-{c[1]}-{'f64' if c[2] else 'f32'}-{'x'.join(map(str, c[3]))}-sched{c[4]}"


def _tune(st, sched, wrap=0):
    t = st.StencilTune()
    t.x3sched = sched
    t.wrap = wrap
    return t


def _model(st, kind, size, fp64, sched, wrap_self):
    cls, kw = (st.Jacobi3D, {}) if kind == "jacobi" else (st.AstarothSim, {"quantities": 1})
    m = cls(size, gpus=[0], temporal=3, fp64=fp64, tune=_tune(st, sched), wrap_self=wrap_self, **kw)
    m.init()
    return m


def _field(size, fp64, seed):
    return torch.rand((size[2], size[1], size[0]), device="cuda", dtype=torch.float64 if fp64 else torch.float32,
                      generator=torch.Generator(device="cuda").manual_seed(seed))


def _assert_schedule(st, dd, kind, tune, form, ragged, expect):
    """The launch stencil7x3_apply makes for sub-domain 0 of dd is the one the case is about."""
    jac = kind == "jacobi"
    k = st.StencilKind.Jacobi if jac else st.StencilKind.Astaroth
    info = stencil7x3_launch_info(dd, 0, 0, k, spheres=jac, tune=tune)
    rounds, parts, blocks = expect
    assert info["supported"] and info["form"] == form and info["ragged"] == ragged, info
    assert info["slots"] == 256, f"the case is sized for 256 resident blocks: {info}"
    nz = dd.domain(0).size().z
    xh = _C.stencil7x3_schedule(True, info["cols"], nz, info["slots"], tune, False)
    assert xh == (3, parts, blocks, rounds), f"rounds schedule of {info['cols']} columns x {nz} planes: {xh}, {info}"
    if form == "xh":
        assert (info["seg"], info["rounds"], info["parts"], info["blocks"]) == (3, rounds, parts, blocks), info
        assert info["blocks"] // info["parts"] * info["rounds"] >= info["cols"], info
    else:
        # the whole-row kernel has no round loop: lockstep parts plus second segments, or the balanced split
        assert info["rounds"] == 1 and info["seg"] in (1, 2), f"whole rows on a rounds schedule: {info}"
        assert 1 <= info["blocks"] <= info["slots"] and (info["seg"] == 1 or info["parts"] >= 2), info
    return info


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_triples_on_the_rounds_threshold_model(st, case):
    """The model (one sub-domain on GPU 0, temporal=3): a triple, triples plus a single-step remainder, and a pair,
    bitwise equal to single steps of the torch oracle after each run."""
    form, kind, fp64, size, sched, wrap_self, wrap, ragged, runs, expect = case
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    m = _model(st, kind, size, fp64, sched, wrap_self)
    assert m.temporal_triples() and m.wrap_axes() == wrap, f"triples {m.temporal_triples()} wrap {m.wrap_axes()}"
    _assert_schedule(st, m.domain, kind, _tune(st, sched, wrap), form, ragged, expect)
    u = _field(size, fp64, 13)
    m.interior(0, 0).copy_(u)
    torch.cuda.synchronize()
    for n in runs:
        m.run(n)
        for _ in range(n):
            u = ref(u)
        m.synchronize()
        got = m.interior(0, 0)
        bad = int((got != u).sum())
        assert bad == 0, f"run({n}): {bad} of {u.numel()} cells differ, max {(got - u).abs().max().item()}"


SENTINEL = 0x7FC0DEAD


def _sweep_next_and_compare(st, dd, u, tune):
    """One stencil7x3_apply on sub-domain 0 with `next` pre-filled with a NaN bit pattern: every interior cell is three
    oracle steps (so none keeps the sentinel: the sweep wrote all of them), every other cell keeps the sentinel."""
    d = dd.domain(0)
    r, sz = d.radius(), d.size()
    nxt = torch.from_dlpack(dd.dlpack(0, 0, False))
    nxt.view(torch.int32).fill_(SENTINEL)
    torch.cuda.synchronize()
    assert stencil7x3_apply(dd, 0, 0, st.StencilKind.Astaroth, spheres=False, tune=tune)
    torch.cuda.synchronize()

    def interior(t):
        return t[r.z(-1):r.z(-1) + sz.z, r.y(-1):r.y(-1) + sz.y, r.x(-1):r.x(-1) + sz.x]

    want = astaroth_step_reference(astaroth_step_reference(astaroth_step_reference(u)))
    got = interior(nxt)
    unwritten = int((interior(nxt.view(torch.int32)) == SENTINEL).sum())
    assert unwritten == 0, f"{unwritten} of {want.numel()} interior cells of next were not written"
    assert torch.equal(got, want), f"{int((got != want).sum())} interior cells differ"
    outside = nxt.view(torch.int32).clone()
    interior(outside).fill_(SENTINEL)
    touched = int((outside != SENTINEL).sum())
    assert touched == 0, f"{touched} cells outside the compute region were written"


def test_whole_row_triple_writes_every_cell_and_nothing_else(st):
    """ops.stencil7x3_apply on the model's own domain of whole periodic 512-cell rows (tune.wrap = 7: every neighbour
    read in-kernel, no halo needed) with 257 row groups on 256 resident blocks."""
    size = (512, 1539, 32)
    m = _model(st, "astaroth", size, False, 1, True)
    assert m.wrap_axes() == 7
    t = _tune(st, 1, 7)
    assert stencil7x3_supported(m.domain, 0, 0, t)
    _assert_schedule(st, m.domain, "astaroth", t, "wrap", False, (3, 2, 172))
    u = _field(size, False, 17)
    m.interior(0, 0).copy_(u)
    torch.cuda.synchronize()
    _sweep_next_and_compare(st, m.domain, u, t)


def test_xh_rounds_triple_writes_every_cell_and_nothing_else(st):
    """ops.stencil7x3_apply on a user's domain (face radius 3, edges and corners 1, every neighbour from the exchanged
    halos): 258 whole columns in 3 rounds of 2 z parts, the last round partly filled."""
    size = (1024, 771, 32)
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_radius(st.Radius.face_edge_corner(3, 1, 1))
    dd.set_gpus([0])
    q = dd.add_data("u", torch.float32)
    dd.realize()
    t = _tune(st, 1, 0)
    assert q == 0 and stencil7x3_supported(dd, 0, q, t)
    _assert_schedule(st, dd.native, "astaroth", t, "xh", False, (3, 2, 172))
    u = _field(size, False, 19)
    dd.curr_interior(0, q).copy_(u)
    torch.cuda.synchronize()
    dd.exchange()
    _sweep_next_and_compare(st, dd.native, u, t)
