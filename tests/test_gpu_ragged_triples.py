"""Fused triples on ragged x extents (stencil7x3_xh_kernel with a partial last column): x extents that are no multiple
of the column width (512 fp32 / 256 fp64 cells), from the kernel up to the model and the ops layer. Every case is
bitwise against the torch oracle. Sizes are (x, y, z)."""
import os

import pytest
import torch

from conftest import run_ranks
from stencil2_amd.ops import astaroth_step_reference, jacobi_step_reference

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "mp_worker.py")


def _model(st, kind, size, fp64=False, gpus=(0,), cost=None, quantities=2, **kw):
    cls, ref = (st.Jacobi3D, jacobi_step_reference) if kind == "jacobi" else (st.AstarothSim, astaroth_step_reference)
    if kind != "jacobi":
        kw["quantities"] = quantities
    if cost is not None:
        kw["axis_cost"] = cost
    m = cls(size, gpus=list(gpus), temporal=3, fp64=fp64, **kw)
    m.init()
    return m, ref, kw.get("quantities", 1)


def _field(size, fp64, seed, scale=1.0):
    dt = torch.float64 if fp64 else torch.float32
    return torch.rand((size[2], size[1], size[0]), device="cuda", dtype=dt,
                      generator=torch.Generator(device="cuda").manual_seed(seed)) * scale


def _set_field(m, u, nq):
    for di in range(m.domain.num_domains()):
        d = m.domain.domain(di)
        o, s = d.origin(), d.size()
        for q in range(nq):
            m.interior(di, q).copy_(u[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x])
    torch.cuda.synchronize()


def _gather(m, q, like):
    g = torch.empty_like(like)
    for di in range(m.domain.num_domains()):
        d = m.domain.domain(di)
        o, s = d.origin(), d.size()
        g[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.interior(di, q)
    return g


def _run_and_compare(m, ref, nq, u, runs):
    for n in runs:
        m.run(n)
        for _ in range(n):
            u = ref(u)
        m.synchronize()
        for q in range(nq):
            got = _gather(m, q, u)
            bad = int((got != u).sum())
            assert bad == 0, f"run({n}) q{q}: {bad} cells differ, max {(got - u).abs().max().item()}"
    return u


RAGGED = [
    # fp32 Astaroth: the chunk that straddles the row end, r % 4 = 0 .. 3
    ("astaroth", (20, 13, 17), False, [0], None, 1.0), ("astaroth", (21, 12, 16), False, [0], None, 1.0),
    ("astaroth", (22, 12, 16), False, [0], None, 1.0), ("astaroth", (23, 12, 16), False, [0], None, 1.0),
    # the boundary between a lane's two chunks
    ("astaroth", (255, 12, 16), False, [0], None, 1.0), ("astaroth", (256, 12, 16), False, [0], None, 1.0),
    ("astaroth", (257, 12, 16), False, [0], None, 1.0),
    # the largest partial column (509 = CW - 3), a whole column plus one cell, the ladder's widths
    ("astaroth", (509, 12, 16), False, [0], None, 1.0), ("astaroth", (513, 12, 16), False, [0], None, 1.0),
    ("astaroth", (323, 20, 24), False, [0], None, 1.0), ("astaroth", (645, 20, 24), False, [0], None, 1.0),
    ("astaroth", (813, 20, 24), False, [0], None, 1.0), ("astaroth", (1029, 13, 17), False, [0], None, 1.0),
    # fp32 Jacobi: spheres of radius nx / 10 centred in y and z, at least 3 cells from every face; tiny sums
    ("jacobi", (323, 72, 72), False, [0], None, 1.0), ("jacobi", (645, 136, 136), False, [0], None, 1.0),
    ("jacobi", (323, 72, 72), False, [0], None, 1e-33),
    # fp64 (256-cell columns)
    ("astaroth", (129, 12, 16), True, [0], None, 1.0), ("astaroth", (253, 12, 16), True, [0], None, 1.0),
    ("astaroth", (300, 20, 24), True, [0], None, 1.0), ("jacobi", (323, 72, 72), True, [0], None, 1.0),
    # several sub-domains on one GPU: x cut (cost 1, 4, 4), y cut (cost 100, 2, 3)
    ("astaroth", (645, 30, 20), False, [0, 0], (1, 4, 4), 1.0),
    ("astaroth", (1290, 24, 20), False, [0, 0, 0, 0], (1, 4, 4), 1.0),
    ("astaroth", (645, 240, 24), False, [0, 0], (100, 2, 3), 1.0),
]


@pytest.mark.parametrize("kind,size,fp64,gpus,cost,scale", RAGGED)
def test_ragged_triples_model(st, kind, size, fp64, gpus, cost, scale):
    """The model on ragged x extents, every halo copied by one depth-3 exchange per triple (wrap_self=False): fused
    triples (the XH kernel with a partial last column), bitwise equal to single steps of the torch oracle through
    graph blocks, triples and the pair / single-step remainders."""
    m, ref, nq = _model(st, kind, size, fp64, gpus, cost, wrap_self=False)
    assert m.temporal_triples() and m.wrap_axes() == 0, f"triples {m.temporal_triples()} wrap {m.wrap_axes()}"
    m.prepare()
    u = _field(size, fp64, 7, scale)
    _set_field(m, u, nq)
    _run_and_compare(m, ref, nq, u, (3, 7, 2, 20, 1))


def test_ragged_triples_more_row_groups_than_blocks(st):
    """More (row group, column) pairs than resident blocks (the schedule's rounds of whole column groups): the ragged
    1029-cell row (3 x 117 = 351 columns) and the whole-column control of 1024 cells (2 x 129 = 258 columns: with 700
    rows it would have 234, fewer than the 256 resident blocks, and run the balanced split). Both are asserted to
    launch rounds (ops.stencil7x3_launch_info)."""
    from stencil2_amd.ops import stencil7x3_launch_info
    for size, cols in (((1024, 771, 16), 258), ((1029, 700, 16), 351)):
        m, ref, nq = _model(st, "astaroth", size, quantities=1, wrap_self=False)
        assert m.temporal_triples() and m.wrap_axes() == 0, f"{size}: triples {m.temporal_triples()}"
        t = st.StencilTune()
        t.wrap = 0
        info = stencil7x3_launch_info(m.domain, 0, 0, st.StencilKind.Astaroth, spheres=False, tune=t)
        assert info["form"] == "xh" and info["ragged"] == (size[0] % 512 != 0) and info["cols"] == cols, info
        assert info["cols"] > info["slots"] and info["seg"] == 3 and info["rounds"] > 1, f"{size}: no rounds: {info}"
        assert info["blocks"] // info["parts"] * info["rounds"] >= cols and info["blocks"] <= info["slots"], info
        u = _field(size, False, 7)
        _set_field(m, u, nq)
        _run_and_compare(m, ref, nq, u, (3, 7, 2, 20, 1))
        del m


@pytest.mark.parametrize("size", [(645, 20, 24), (813, 20, 24)])
def test_ragged_triples_default_policy(st, size):
    """One GPU, wrap_self default, the weak-scaling ladder's row widths: the measured exception. The fused pairs wrap
    these rows in-kernel and beat the ragged triples on most ladder shapes (one MI355X, Gcells/s triples vs pairs:
    645x645x323 940-960 vs 1072-1078, 645x323x645 983-987 vs 1098-1138, 323x645x645 940-992 vs 1005-1020, 813x813x204
    978-993 vs 1039-1053; triples ahead only on 813x407x407, 1041-1047 vs 960-983, and 407x407x813, 1184-1211 vs
    1126-1133), so
    the model keeps the pairs and every in-kernel wrap for rows the pair kernel wraps (stencil_model.cpp)."""
    m, ref, nq = _model(st, "astaroth", size)
    assert not m.temporal_triples() and m.temporal_blocking() and m.wrap_axes() == 7, \
        f"triples {m.temporal_triples()} wrap {m.wrap_axes()}"
    u = _field(size, False, 9)
    _set_field(m, u, nq)
    _run_and_compare(m, ref, nq, u, (3, 7, 2, 20, 1))


@pytest.mark.parametrize("size,fp64", [((510, 12, 16), False), ((511, 12, 16), False), ((1023, 12, 16), False),
                                       ((255, 12, 16), True)])
@pytest.mark.parametrize("wrap_self", [False, True])
def test_ragged_triples_policy_edge(st, size, fp64, wrap_self):
    """Rows ending 1 or 2 cells short of a whole column (and their neighbours): whichever kernel the model picks, the
    result is bitwise the oracle's, and temporal_triples() agrees with ops.stencil7x3_supported for the model's
    sub-domain and wrap mask."""
    from stencil2_amd.ops import stencil7x3_supported
    m, ref, nq = _model(st, "astaroth", size, fp64, wrap_self=wrap_self)
    t = st.StencilTune()
    t.wrap = m.wrap_axes()
    for q in range(nq):
        assert m.temporal_triples() == stencil7x3_supported(m.domain, 0, q, t), f"wrap {m.wrap_axes()}"
    u = _field(size, fp64, 3)
    _set_field(m, u, nq)
    _run_and_compare(m, ref, nq, u, (3, 7, 2, 20, 1))


def _ops_domain(st, size, dtype, face):
    dd = st.DistributedDomain(*size, group=st.make_single_group())
    dd.set_radius(st.Radius.face_edge_corner(face, 1, 1))
    dd.set_gpus([0])
    q = dd.add_data("u", dtype)
    dd.realize()
    return dd, q


@pytest.mark.parametrize("size,fp64", [((21, 13, 17), False), ((323, 20, 24), False), ((645, 13, 17), False),
                                       ((129, 13, 17), True)])
def test_ragged_triple_stores_stay_inside_the_region(st, size, fp64):
    """ops.stencil7x3_apply on a user's domain (face radius 3, edges and corners 1): the interior of `next` is three
    oracle steps, and every other cell of `next` (halos, the +x halo beside the ragged column included, and padding)
    keeps the bit pattern it held before the call."""
    from stencil2_amd.ops import stencil7x3_apply, stencil7x3_supported
    dtype, itype = (torch.float64, torch.int64) if fp64 else (torch.float32, torch.int32)
    dd, q = _ops_domain(st, size, dtype, 3)
    t = st.StencilTune()
    t.wrap = 0
    assert stencil7x3_supported(dd, 0, q, t)
    u = _field(size, fp64, 11)
    dd.curr_interior(0, q).copy_(u)
    torch.cuda.synchronize()
    dd.exchange()
    sentinel = 0x7FC0DEAD7FC0DEAD if fp64 else 0x7FC0DEAD
    nxt = dd.next(0, q)
    nxt.view(itype).fill_(sentinel)
    torch.cuda.synchronize()
    assert stencil7x3_apply(dd, 0, q, st.StencilKind.Astaroth, spheres=False, tune=t)
    torch.cuda.synchronize()
    want = astaroth_step_reference(astaroth_step_reference(astaroth_step_reference(u)))
    got = dd.interior(nxt, 0)
    assert torch.equal(got, want), f"{int((got != want).sum())} interior cells differ"
    outside = nxt.view(itype).clone()
    dd.interior(outside, 0).fill_(sentinel)
    touched = int((outside != sentinel).sum())
    assert touched == 0, f"{touched} cells outside the compute region were written"


def test_ragged_triple_refuses_shallow_halos(st):
    """Face radius 2: stencil7x3_supported is false and stencil7x3_apply returns False without launching (next keeps
    its bits)."""
    from stencil2_amd.ops import stencil7x3_apply, stencil7x3_supported
    dd, q = _ops_domain(st, (323, 20, 24), torch.float32, 2)
    t = st.StencilTune()
    t.wrap = 0
    assert not stencil7x3_supported(dd, 0, q, t)
    nxt = dd.next(0, q)
    nxt.view(torch.int32).fill_(0x7FC0DEAD)
    torch.cuda.synchronize()
    assert stencil7x3_apply(dd, 0, q, st.StencilKind.Astaroth, spheres=False, tune=t) is False
    torch.cuda.synchronize()
    assert int((nxt.view(torch.int32) != 0x7FC0DEAD).sum()) == 0


# cuts follow the interface cost (NodePartition): x (1,4,4). With 645-cell rows the costs (4,2,3) / (4,3,2) that cut
# 512 x 300 x 24 / 512 x 16 x 300 along y / z cut x instead (4 Y Z < 2 X Z), so x is priced out: y (100,2,3), z (100,3,2)
@pytest.mark.parametrize("kind,size,ranks,cost,wrap,toggle", [
    ("astaroth", "645,36,40", 2, "1,4,4", "6", None), ("jacobi", "645,136,136", 2, "1,4,4", "6", None),
    ("astaroth", "1290,24,20", 4, "1,4,4", "6", None),
    # y / z cut: remote halos and no x cut, so the model starts with overlapped pairs; mode 0 (whole regions) takes
    # the triples, mode 4 the pipelined triples (as test_triples_across_ranks)
    ("astaroth", "645,300,24", 2, "100,2,3", "4", "0"), ("astaroth", "645,16,300", 2, "100,3,2", "2", "0")])
def test_ragged_triples_across_ranks(kind, size, ranks, cost, wrap, toggle):
    """Ragged rows on ranks sharing one GPU over HIP IPC: x cut (every rank's last column partial, x halos from the
    neighbour rank), y cut and z cut (whole-region triples, overlap mode 0). Bitwise vs the oracle."""
    _ranks_case(kind, size, ranks, cost, wrap, toggle)


def _ranks_case(kind, size, ranks, cost, wrap, toggle):
    env = {"MP_DEVICE": "1", "MP_METHODS": "All", "STENCIL_WAIT_TIMEOUT": "20", "MP_TEMPORAL": "3", "MP_KIND": kind,
           "MP_RANDOM": "1", "MP_AXIS_COST": cost, "MP_RUN_STEPS": "9", "MP_EXPECT_TRIPLES": "1",
           "MP_EXPECT_WRAP": wrap}
    if toggle is not None:
        env.update({"MP_TOGGLE_OVERLAP": "1", "MP_TOGGLE_MODES": toggle, "MP_TOGGLE_STEPS": "10"})
    outs = run_ranks(ranks, WORKER, ["jacobi", size], env_extra=env)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
        assert "jacobi bad 0" in out, out[-2000:]


def test_ragged_pipelined_triples_across_ranks():
    """z cut with pipelined triples (overlap mode 4: the depth-3 exchange gated on the cells the previous triple
    published, which a partial column counts by its own width). Triples on a 645-cell row read x from halos, so the
    x self copies stay in the exchange as same-GPU translate copies; they read every plane of the sweep, which the
    gate does not certify, so the gated exchange runs them last, behind the whole sweep
    (DistributedDomain::gated_send_supported with translate copies), while its sends and receives start on the
    published planes."""
    _ranks_case("astaroth", "645,16,300", 2, "100,3,2", "2", "4")
