"""The whole-row fused triple (stencil7x3_wrap_kernel) where a change to the VALU work of its z step can break it.

Written with the "VALU diet" experiments ("VALU diet of the whole-row triple"; profiles/valu_diet/): a
lane layout of 8 consecutive cells, one tiny-sum test per row update, compile-time LDS buffer indices, and the 12-phase
unroll the analysis found unnecessary. What such changes can break, and what these tests pin on the kernel as it is:

  * the end of a march at every phase of an unrolled loop (up to 12 phases: a march of n planes runs n + 4 steps, so
    n + 4 mod 12 must take every value), in both march directions, with a second march of the same block behind it;
  * rows past the y end (y = 6: one full row group, y = 8 and 14: a 2-row partial group that stores into the sink);
  * the x wrap partner and the chunk order (a field that encodes (x, y, z) exactly, so cells 0, 255, 256 and 511 of
    every row differ);
  * the tiny-sum branch of the exact /6 at each of the three levels alone and together: sums in (0, 2^-100) from
    values in [2^-126, 2^-102], denormals and exact zeros in bands of rows next to ordinary rows, Jacobi (a band that
    crosses the spheres and one that does not) and Astaroth. The CPU tests assert that the oracle itself meets such
    sums at each level on these fields.

The kernel takes fp32 rows of exactly 512 cells and fields of at least 16 planes (stencil7x3_supported), so the issue's
z extents 1 .. 5, 11, 12, 13 and 25 are lengths of marches (the planes one block sweeps in one go), not grid extents:
test_plan_holds_the_marches asserts through _C.stencil7x3_plan that the grids used here hold marches of exactly those
lengths, every exit phase mod 12 in both directions, and blocks with more than one march. Every comparison is bitwise
(torch.equal) against the pure-torch oracle, computed once per field and shared."""
import functools

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import astaroth_step_reference, jacobi_step_reference

# x3sched, x3parts, x2lockstep, alternate_z
BALANCED, BALANCED_NOALT, PARTS2 = (0, 0, 1, 1), (0, 0, 1, 0), (1, 2, 1, 1)
# (512, 73, 29) balanced over 256 blocks: marches of 1 .. 5, 11, 12, 13 and 25 planes, every n + 4 mod 12, up and down
MARCH_GRID = (512, 73, 29)
MARCH_LENGTHS = {1, 2, 3, 4, 5, 11, 12, 13, 25}
# the issue's y = 12 with marches of 25 (one per row group), 12 / 13 / 24 / 25, and two z parts of 25 planes
Y12_GRIDS = (((512, 12, 25), BALANCED), ((512, 12, 37), BALANCED), ((512, 12, 50), PARTS2))
Y_GRIDS = ((512, 6, 25), (512, 8, 25), (512, 14, 25))
JACOBI_GRID = (512, 107, 108)  # the smallest grids whose spheres stay clear of the periodic faces fuse triples
TINY = 2.0 ** -100


def _tune(variant):
    t = _C.StencilTune()
    t.x3sched, t.x3parts = variant[0], variant[1]
    t.x2lockstep = type(t.x2lockstep)(variant[2])
    t.alternate_z = bool(variant[3])
    return t


def _marches(size, jacobi, variant):
    m = _C.stencil7x3_plan(size, jacobi, _tune(variant)).marches
    assert len(m) % 5 == 0
    return [tuple(m[i:i + 5]) for i in range(0, len(m), 5)]  # block, row group, first plane, planes, down


def test_plan_holds_the_marches():
    ms = _marches(MARCH_GRID, False, BALANCED)
    assert MARCH_LENGTHS <= {n for _, _, _, n, _ in ms}
    for down in (False, True):
        exits = {(n + 4) % 12 for _, _, _, n, d in ms if bool(d) == down}
        assert exits == set(range(12)), (down, sorted(exits))
    blocks = [b for b, *_ in ms]
    assert len(blocks) > len(set(blocks)), "no block with a second march"
    assert {n for _, _, _, n, _ in _marches((512, 12, 25), False, BALANCED)} == {25}
    assert {12, 13, 25} <= {n for _, _, _, n, _ in _marches((512, 12, 37), False, BALANCED)}
    two = _marches((512, 12, 50), False, PARTS2)
    assert {n for _, _, _, n, _ in two} == {25} and len(two) == 4  # 2 row groups x 2 z parts
    assert {bool(d) for *_, d in two} == {False, True}
    for size in Y_GRIDS:  # y = 8, 14: the last row group holds 2 rows
        assert {g for _, g, *_ in _marches(size, False, BALANCED)} == set(range((size[1] + 5) // 6))


# ---- fields ----
def coordinate_field(size):
    """a value per cell that encodes (x, y, z) exactly in fp32 (below 2^24): every cell of the grid differs"""
    X, Y, Z = size
    assert X * Y * Z < 2 ** 24
    z = torch.arange(Z, dtype=torch.float32).view(-1, 1, 1)
    y = torch.arange(Y, dtype=torch.float32).view(1, -1, 1)
    x = torch.arange(X, dtype=torch.float32).view(1, 1, -1)
    return (z * Y + y) * X + x + 1


def band_rows(size, centre):
    return [(centre + d) % size[1] for d in range(-3, 4)]


def tiny_field(size, centres, seed):
    """Ordinary values in [0, 1) except in bands of 7 rows around each row of `centres` (y wraps). All rows of a band
    share one class per plane, drawn per band: ordinary, exact zeros, or tiny values (|u| in [2^-126, 2^-102], a
    quarter of them denormals). A sum of the band's centre row is then in (0, 2^-100) at level k where the planes
    around it held only zeros and tiny values for k steps, which happens per level alone and for all three at once
    (tiny_levels; asserted by the CPU tests). One further row holds denormals only, between ordinary rows."""
    X, Y, Z = size
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((Z, Y, X), generator=g)
    for centre in centres:
        cls = torch.randint(0, 5, (Z,), generator=g)  # 0: ordinary, 1 - 2: zeros, 3 - 4: tiny
        expo = torch.randint(-126, -101, (Z, 7, X), generator=g).to(torch.float32)
        tiny = torch.exp2(expo) * (1 + torch.rand((Z, 7, X), generator=g))
        den = torch.randint(1, 2 ** 20, (Z, 7, X), generator=g).to(torch.float32) * 2.0 ** -149
        tiny = torch.where(torch.rand((Z, 7, X), generator=g) < 0.25, den, tiny)
        for i, y in enumerate(band_rows(size, centre)):
            row = torch.where((cls >= 3).view(-1, 1), tiny[:, i, :], torch.zeros(Z, X))
            u[:, y, :] = torch.where((cls == 0).view(-1, 1), u[:, y, :], row)
    lone = (centres[0] + 5) % Y
    u[:, lone, :] = torch.randint(1, 2 ** 23, (Z, X), generator=g).to(torch.float32) * 2.0 ** -149
    assert bool((u[:, lone, :] < 2.0 ** -126).all()) and bool((u[:, lone, :] > 0).all())
    return u


def six_sum(kind, u):
    """the six-term sum of the reference step, in its order"""
    nb = {"px": torch.roll(u, -1, 2), "mx": torch.roll(u, 1, 2), "py": torch.roll(u, -1, 1),
          "my": torch.roll(u, 1, 1), "pz": torch.roll(u, -1, 0), "mz": torch.roll(u, 1, 0)}
    order = ("px", "mx", "py", "my", "pz", "mz") if kind == "jacobi" else ("mx", "my", "mz", "px", "py", "pz")
    s = torch.zeros_like(u)
    for k in order:
        s = s + nb[k]
    return s


def tiny_levels(kind, u):
    """per level 1 .. 3, the (plane, row) pairs of the oracle's run on u that hold a sum in (0, 2^-100)"""
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    out = []
    for _ in range(3):
        s = six_sum(kind, u)
        out.append((((s.abs() < TINY) & (s != 0)).any(dim=2)))
        u = ref(u)
    return out


def level_sets(kind, u, row):
    """the sets of levels whose tiny-sum branch one z step of the output row `row` takes, per march direction: the
    step that stores plane z computes level 1 at plane z + 2 dz, level 2 at z + dz and level 3 at z"""
    m1, m2, m3 = (m[:, row] for m in tiny_levels(kind, u))
    Z = m1.numel()
    seen = {1: set(), -1: set()}
    for dz in (1, -1):
        for z in range(Z):
            hit = frozenset(k for k, m, p in ((1, m1, z + 2 * dz), (2, m2, z + dz), (3, m3, z)) if bool(m[p % Z]))
            seen[dz].add(hit)
    return seen


WANTED_SETS = {frozenset({1}), frozenset({2}), frozenset({3}), frozenset({1, 2, 3})}
TINY_CASES = {  # kind -> grid, band centres (Jacobi: row 53 crosses both spheres, rows 105 .. 1 touch none), seed
    "astaroth": ((512, 12, 64), (5,), 12),
    "jacobi": (JACOBI_GRID, (53, 106), 10),
}


@pytest.mark.parametrize("kind", ["astaroth", "jacobi"])
def test_oracle_takes_the_true_division_at_each_level(kind):
    size, centres, seed = TINY_CASES[kind]
    u = tiny_field(size, centres, seed)
    for k, m in enumerate(tiny_levels(kind, u), 1):
        assert bool(m.any()), f"no sum in (0, 2^-100) at level {k}"
    for c in centres:
        seen = level_sets(kind, u, c)
        for dz in (1, -1):
            assert WANTED_SETS <= seen[dz], (kind, c, dz, sorted(map(sorted, seen[dz])))
    if kind == "jacobi":
        from stencil2_amd.ops import jacobi_spheres
        hot, cold, R = jacobi_spheres(size)
        assert abs(centres[0] - hot[1]) <= R  # the first band crosses the spheres
        for y in ((centres[1] + d) % size[1] for d in (-1, 0, 1, 2)):  # the second band's inner rows touch none
            assert (y - hot[1]) ** 2 >= (R + 1) ** 2 and (y - cold[1]) ** 2 >= (R + 1) ** 2


# ---- GPU ----
@functools.lru_cache(maxsize=None)
def _case(kind, size, field):
    """the start field and the oracle after one and two triples (CPU, shared, never modified)"""
    if field == "coordinate":
        u0 = coordinate_field(size)
    elif field == "tiny":
        u0 = tiny_field(size, *TINY_CASES[kind][1:])
    else:
        u0 = torch.rand((size[2], size[1], size[0]), generator=torch.Generator().manual_seed(41))
    ref = jacobi_step_reference if kind == "jacobi" else astaroth_step_reference
    want, u = [], u0
    for _ in range(2):
        for _ in range(3):
            u = ref(u)
        want.append(u)
    return u0, want


def _run(st, kind, size, variant, field):
    """two triples (the second on the odd buffer parity, where alternate_z flips every march), each bitwise equal"""
    u0, want = _case(kind, size, field)
    cls, kw = (st.Jacobi3D, {}) if kind == "jacobi" else (st.AstarothSim, {"quantities": 1})
    m = cls(size, gpus=[0], temporal=3, tune=_tune(variant), **kw)
    m.init()
    assert m.temporal_triples() and m.wrap_axes() == 7, (m.temporal_triples(), m.wrap_axes())
    m.prepare()
    m.interior(0, 0).copy_(u0.cuda())
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        m.run(3)
        m.synchronize()
        got = m.interior(0, 0).cpu()
        assert torch.equal(got, w), (f"triple {i}: {int((got != w).sum())} of {w.numel()} cells differ, first at "
                                     f"(z, y, x) = {tuple((got != w).nonzero()[0].tolist())}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [BALANCED, BALANCED_NOALT], ids=["alt", "noalt"])
@pytest.mark.parametrize("field", ["random", "coordinate"])
def test_every_exit_phase(st, variant, field):
    _run(st, "astaroth", MARCH_GRID, variant, field)


@pytest.mark.gpu
@pytest.mark.parametrize("size,variant", Y12_GRIDS, ids=lambda v: "x".join(map(str, v)))
def test_y12_marches_and_z_parts(st, size, variant):
    _run(st, "astaroth", size, variant, "coordinate")
    if variant[3]:
        _run(st, "astaroth", size, variant[:3] + (0,), "coordinate")


@pytest.mark.gpu
@pytest.mark.parametrize("size", Y_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_y_extents_and_the_sink(st, size):
    _run(st, "astaroth", size, BALANCED, "coordinate")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["astaroth", "jacobi"])
@pytest.mark.parametrize("variant", [BALANCED, BALANCED_NOALT, (1, 0, 1, 1)], ids=["alt", "noalt", "parts"])
def test_tiny_sums_at_each_level(st, kind, variant):
    _run(st, kind, TINY_CASES[kind][0], variant, "tiny")


@pytest.mark.gpu
def test_jacobi_wrap_partners(st):
    """Jacobi on the coordinate field: the spheres cross the rows of the middle row groups and miss the outer ones"""
    u0, _ = _case("jacobi", JACOBI_GRID, "coordinate")
    assert len({float(u0[3, 5, x]) for x in (0, 255, 256, 511)}) == 4
    _run(st, "jacobi", JACOBI_GRID, BALANCED, "coordinate")
