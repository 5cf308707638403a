"""The ends of the z marches of the whole-row fused triples (stencil7x3_wrap_kernel), and both of its store forms.

Written with an experiment that kept each output plane in registers across the barrier and stored it one z step
later, behind the next load wait, with a flush after a march's last step (measured slower and not merged: BASELINE.md,
"Deferred output stores"). What such a change can break is what these tests pin on the kernel as it is: the end of a
march (a plane stored at the wrong z or not at all: marches of 1, 2 or 3 planes, a loop left at any of its four
unrolled phases, a march followed by another of the same block), rows past the y end (the sink), and writes outside
the compute region. The kernel compiles an instance per StencilTune::nontemporal setting; both run here.

Every comparison is bitwise against the torch oracle. Sizes are (x, y, z), mostly 512 x <= 40 x <= 40 cells; the
schedule variants are the tune fields that change how the (row group, plane) space is cut into marches. The plan test
(CPU) asserts through _C.stencil7x3_plan(...).marches that the sweep really holds marches of 1, 2 and 3 planes, every
length residue mod 4, both directions and both z faces, followed by another march of the same block. The plan is for
256 resident blocks (one MI355X), which the GPU tests assert of the device they run on."""
import itertools

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (astaroth_step_reference, jacobi_step_reference, stencil7x3_apply, stencil7x3_launch_info,
                              stencil7x3_supported)

NYS = (3, 7, 13, 20, 38)
NZS = (16, 17, 18, 19, 21, 23, 37)
# On 256 resident blocks the balanced split gives a block about 24 planes, so the grid above holds no march shorter than
# 3 planes (the plan test found that). The smallest y extents that do: marches of 1 plane followed by another march of
# the block, down (145, 16) and up (139, 17), and of 2 planes, down (73, 16) and up (73, 17)
EXTRA = ((145, 16), (139, 17), (73, 16), (73, 17))
YZ = tuple(itertools.product(NYS, NZS)) + EXTRA
# Jacobi: the model fuses triples only where the spheres (radius x / 10 around the centre of y and z) stay 2 / 3 cells
# clear of the periodic faces, which needs y, z >= 107 for 512-cell rows; thinner Jacobi grids run single steps. So the
# Jacobi instances run on the smallest such grids, one z extent per residue mod 4 (lockstep parts, sphere-weighted)
YZ_JACOBI = ((107, 108), (107, 109), (109, 110), (110, 111))
RUNS = (3, 6, 2, 1)  # triples, triples, the pair, a single step
# x3sched, x3parts, x2lockstep, alternate_z
VARIANTS = list(itertools.product((0, 1), (0, 2, 3), (0, 1), (0, 1)))


def _tune(variant, wrap=0, nontemporal=True):
    t = _C.StencilTune()
    t.nontemporal = nontemporal
    t.x3sched, t.x3parts = variant[0], variant[1]
    t.x2lockstep = type(t.x2lockstep)(variant[2])
    t.alternate_z = bool(variant[3])
    t.wrap = wrap
    return t


def _marches(size, jacobi, variant):
    m = _C.stencil7x3_plan(size, jacobi, _tune(variant)).marches
    assert len(m) % 5 == 0
    return [tuple(m[i:i + 5]) for i in range(0, len(m), 5)]  # block, row group, first plane, planes, down


def test_sweep_holds_the_marches_it_is_about():
    """The marches of the sweep's cases (whole rows, as stencil7x3_apply cuts them on 256 resident blocks): each case
    covers every (row group, plane) once, and over the sweep there are marches of 1, 2 and 3 planes and of every length
    mod 4, up and down, ending at the low and at the high z face, each kind followed by another march in its block."""
    lengths, residues, followed = set(), set(), set()
    cases = [(yz, False) for yz in YZ] + [(yz, True) for yz in YZ_JACOBI]
    for ((ny, nz), jac), v in itertools.product(cases, VARIANTS):
        ms = _marches((512, ny, nz), jac, v)
        cover = sorted((g, z) for _, g, z0, n, _ in ms for z in range(z0, z0 + n))
        assert cover == [(g, z) for g in range((ny + 5) // 6) for z in range(nz)], (ny, nz, jac, v)
        for i, (b, g, z0, n, down) in enumerate(ms):
            assert n >= 1
            lengths.add(n)
            residues.add(n % 4)
            if i + 1 < len(ms) and ms[i + 1][0] == b:
                # the face the march ends at (its last stored plane: the flush), if any
                last = z0 if down else z0 + n - 1
                face = "lo" if last == 0 else ("hi" if last == nz - 1 else "mid")
                followed.add((n if n <= 3 else 4 + n % 4, bool(down), face))  # 1, 2, 3 planes; longer: 4 + n mod 4
    assert {1, 2, 3} <= lengths and residues == {0, 1, 2, 3}, (sorted(lengths), residues)
    kinds = {k for k, _, _ in followed}
    assert set(range(1, 8)) <= kinds, f"march lengths followed by another march of the block: {sorted(kinds)}"
    assert {d for _, d, _ in followed} == {False, True}
    assert {"lo", "hi"} <= {f for _, _, f in followed}, followed


def _model(st, kind, size, variant, nontemporal=True):
    cls, kw = (st.Jacobi3D, {}) if kind == "jacobi" else (st.AstarothSim, {"quantities": 1})
    m = cls(size, gpus=[0], temporal=3, tune=_tune(variant, nontemporal=nontemporal), **kw)
    m.init()
    return m


def _field(size, seed):
    return torch.rand((size[2], size[1], size[0]), device="cuda",
                      generator=torch.Generator(device="cuda").manual_seed(seed))


def _oracle(kind, u):
    """the field after each of RUNS (computed once per case, shared by its schedule variants, never modified)"""
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    out = []
    for n in RUNS:
        for _ in range(n):
            u = ref(u)
        out.append(u)
    return out


def _run_variants(st, kind, size, nontemporal=True):
    u0 = _field(size, 23)
    want = _oracle(kind, u0)
    sk = st.StencilKind.Jacobi if kind == "jacobi" else st.StencilKind.Astaroth
    for v in VARIANTS:
        m = _model(st, kind, size, v, nontemporal)
        assert m.temporal_triples() and m.wrap_axes() == 7, f"{v}: triples {m.temporal_triples()} wrap {m.wrap_axes()}"
        info = stencil7x3_launch_info(m.domain, 0, 0, sk, spheres=kind == "jacobi", tune=_tune(v, 7, nontemporal))
        assert info["supported"] and info["form"] == "wrap" and info["slots"] == 256, info
        m.prepare()
        m.interior(0, 0).copy_(u0)
        torch.cuda.synchronize()
        for n, w in zip(RUNS, want):
            m.run(n)
            m.synchronize()
            got = m.interior(0, 0)
            bad = int((got != w).sum())
            assert bad == 0, (f"variant (x3sched, x3parts, x2lockstep, alternate_z) = {v}, run({n}): {bad} of "
                              f"{w.numel()} cells differ, max {(got - w).abs().max().item()}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ny,nz", [("astaroth", y, z) for y, z in YZ] + [("jacobi", y, z) for y, z in YZ_JACOBI])
def test_wrap_triples_every_march_length(st, kind, ny, nz):
    """Whole periodic rows (one GPU, every axis wrapped in-kernel, nontemporal stores: the default) under every
    schedule variant: triples, the pair and the single-step remainder interleaved, bitwise equal to the oracle after
    each run."""
    _run_variants(st, kind, (512, ny, nz))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ny,nz", [("astaroth", 13, 17), ("astaroth", 38, 37), ("astaroth", 145, 16),
                                        ("astaroth", 73, 17), ("jacobi", 107, 109)])
def test_wrap_triples_plain_stores(st, kind, ny, nz):
    """The instances with plain output stores (StencilTune.nontemporal = False): the same sweep on the shapes that
    hold the shortest marches, the lockstep parts and the Jacobi spheres."""
    _run_variants(st, kind, (512, ny, nz), nontemporal=False)


SENTINEL = 0x7FC0DEAD


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(512, 13, 17), (512, 8, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", [(0, 0, 1, 0), (1, 0, 1, 1)], ids=lambda v: "v" + "".join(map(str, v)))
@pytest.mark.parametrize("nontemporal", [True, False], ids=["nt", "plain"])
def test_wrap_triple_writes_every_cell_and_nothing_else(st, size, variant, nontemporal):
    """One stencil7x3_apply (whole rows) into a destination filled with a NaN bit pattern, halos and row padding
    included: every interior cell is three oracle steps, every byte outside the compute region keeps the pattern. The
    last row group of both shapes has rows past the y end, whose stores go to the sink."""
    m = _model(st, "astaroth", size, variant, nontemporal)
    assert m.wrap_axes() == 7
    t = _tune(variant, 7, nontemporal)
    dd = m.domain
    assert stencil7x3_supported(dd, 0, 0, t)
    u = _field(size, 29)
    m.interior(0, 0).copy_(u)
    d = dd.domain(0)
    r, sz = d.radius(), d.size()
    nxt = torch.from_dlpack(dd.dlpack(0, 0, False))
    nxt.view(torch.int32).fill_(SENTINEL)
    torch.cuda.synchronize()
    assert stencil7x3_apply(dd, 0, 0, st.StencilKind.Astaroth, spheres=False, tune=t)
    torch.cuda.synchronize()

    def interior(x):
        return x[r.z(-1):r.z(-1) + sz.z, r.y(-1):r.y(-1) + sz.y, r.x(-1):r.x(-1) + sz.x]

    want = astaroth_step_reference(astaroth_step_reference(astaroth_step_reference(u)))
    unwritten = int((interior(nxt.view(torch.int32)) == SENTINEL).sum())
    assert unwritten == 0, f"{unwritten} of {want.numel()} interior cells of next were not written"
    got = interior(nxt)
    assert torch.equal(got, want), f"{int((got != want).sum())} interior cells differ"
    outside = nxt.view(torch.int32).clone()
    interior(outside).fill_(SENTINEL)
    touched = int((outside != SENTINEL).sum())
    assert touched == 0, f"{touched} cells outside the compute region were written"
