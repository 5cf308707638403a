"""Cases shared by test_mg.py (host backend) and test_gpu_mg.py (the HIP kernels): the StarMG V-cycle solver.

One cycle is compared bitwise with ops.mg_cycle_reference on the gathered grid. The convergence limits (within 12
cycles to 1e-6, every factor of the first six cycles <= 0.35) come from a torch prototype of the same arithmetic,
whose worst factor was 0.249 and which reached 1e-6 in 9 cycles in every case; they do not come from the code under
test. The reference histories are computed once per case and shared."""
import functools
import math

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (axpby_reference, box_step_reference, box_to_lists, box_weights, laplacian_box,
                              mg_cycle_reference, star_step_reference, star_weights)

from algebra_cases import gather_solution, same_bits
from reduce_cases import random_field

FC = _C.FaceCondition
DTYPES = [torch.float64, torch.float32]


def poisson():
    return star_weights(1, 6.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])  # -Laplacian, 7 points


def helmholtz(s=0.01):
    return star_weights(1, 6.0 + s, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])


def minus_box27():
    return box_weights([[[-v for v in row] for row in plane] for plane in box_to_lists(laplacian_box(27))])


def conditions(x=None, y=None, z=None):
    bc = _C.BoundaryConditions()
    for ax, faces in enumerate((x, y, z)):
        if faces is not None:
            bc.set_axis(ax, *faces)
    return bc


def cycle_walls():
    """mixed walls, antimirror(1.0) on one face: the inhomogeneous value enters at level 0 only"""
    return conditions((FC.antimirror(1.0), FC.mirror()), (FC.mirror(), FC.antimirror(0.0)),
                      (FC.constant(0.25), FC.antimirror(0.0)))


def all_antimirror():
    return conditions(*[(FC.antimirror(0.25), FC.antimirror(0.25))] * 3)


def mixed():
    return conditions((FC.antimirror(0.0), FC.antimirror(0.5)), (FC.mirror(), FC.mirror()), None)


# name -> (weights, boundary, gpus, levels)
CONVERGENCE = {
    "poisson_antimirror": (poisson, all_antimirror, (0,), 4),
    "poisson_antimirror_two": (poisson, all_antimirror, (0, 0), 3),
    "helmholtz_periodic": (helmholtz, lambda: None, (0,), 4),
    "poisson_mixed": (poisson, mixed, (0,), 4),
}
SIZE = (32, 32, 32)


def rhs(size, dtype, seed=91):
    return random_field(tuple(size), dtype, seed)


def make_mg(st, backend, size, w, bc, dtype, gpus=(0,), f=None, group=None, methods=None, **kw):
    if methods is not None:
        kw["methods"] = methods
    m = st.StarMG(size, w, fp64=dtype == torch.float64, gpus=list(gpus), backend=backend, boundary=bc,
                  group=group if group is not None else st.make_single_group(), **kw)
    f = rhs(size, dtype) if f is None else f
    X, Y, Z = size
    m.set_rhs(lambda gz, gy, gx: f.to(gz.device)[gz % Z, gy % Y, gx % X])
    return m, f


def relres(u, f, w, bc):
    """||f - A u||2 / ||f||2: the residual in the fields' type as the solver forms it, the sums in float64"""
    step = box_step_reference if isinstance(w, _C.BoxWeights) else star_step_reference
    r = axpby_reference(1.0, f, -1.0, step(u, w, boundary=bc)).double()
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


# ---- 1. one cycle, bitwise ----
def case_cycle(st, backend, dtype, box):
    w = minus_box27() if box else poisson()
    bc = cycle_walls()
    m, f = make_mg(st, backend, (16, 16, 16), w, bc, dtype, max_levels=3)
    assert m.levels == 3 and level_sizes(m) == [(16,) * 3, (8,) * 3, (4,) * 3]
    m.cycle()
    got = gather_solution(m)
    want = mg_cycle_reference(torch.zeros_like(f), f, [m.level_weights(l) for l in range(m.levels)], bc, m.nu, m.omega,
                              m.coarse_sweeps)
    bad = int((got != want).sum())
    assert same_bits(got, want), f"{dtype} box={box}: {bad} cells differ, max {float((got - want).abs().max()):.3e}"
    assert relres(got, f, w, bc) < 0.35  # and it is a multigrid cycle, not only the same arithmetic


# ---- 2. convergence against the prototype's limits and the reference's history ----
@functools.lru_cache(maxsize=None)
def reference_history(name, dtype, levels, cycles):
    """relres after each of `cycles` reference cycles (computed once per case)"""
    from stencil2_amd.ops import coarsened_weights
    wf, bcf, _, _ = CONVERGENCE[name]
    w, bc = wf(), bcf()
    ws = [coarsened_weights(w, l) for l in range(levels)]
    f = rhs(SIZE, dtype)
    u = torch.zeros_like(f)
    out = []
    for _ in range(cycles):
        u = mg_cycle_reference(u, f, ws, bc, (2, 2), 6.0 / 7.0, 32)
        out.append(relres(u, f, w, bc))
    return tuple(out)


def case_convergence(st, backend, name):
    wf, bcf, gpus, levels = CONVERGENCE[name]
    w, bc, dtype = wf(), bcf(), torch.float64
    m, f = make_mg(st, backend, SIZE, w, bc, dtype, gpus)
    assert m.levels == levels and m.domain.num_domains() == len(gpus), (m.levels, m.domain.num_domains())
    if len(gpus) == 2:
        s = m.level_domain(m.levels - 1).domain(0).size()
        assert sorted((s.x, s.y, s.z)) == [4, 8, 8], s
    cycles, rel = m.solve(tol=1e-6)
    h = m.history
    factors = [h[k + 1] / h[k] for k in range(min(5, len(h) - 1))]
    print(f"{name}: cycles {cycles} relres {rel:.3e} history {['%.3e' % v for v in h]} factors {['%.3f' % v for v in factors]}")
    assert cycles == len(h) <= 12 and rel == h[-1] < 1e-6, (cycles, h)
    assert len(factors) == 5 and all(v <= 0.35 for v in factors), factors
    true = relres(gather_solution(m), f, w, bc)
    assert abs(true - rel) <= 1e-6 * rel + 1e-14, (true, rel)
    ref = reference_history(name, dtype, levels, cycles)
    for k, (a, b) in enumerate(zip(h, ref)):
        assert abs(a - b) <= 1e-6 * b, f"cycle {k + 1}: relres {a!r}, reference {b!r}"
    return m


def case_fp32(st, backend):
    wf, bcf, gpus, levels = CONVERGENCE["poisson_antimirror"]
    m, f = make_mg(st, backend, SIZE, wf(), bcf(), torch.float32, gpus)
    cycles, rel = m.solve(tol=1e-5)
    print(f"fp32: cycles {cycles} relres {rel:.3e} history {['%.3e' % v for v in m.history]}")
    assert m.levels == levels and cycles <= 10 and rel < 1e-5, (cycles, m.history)


# ---- 3. the level rule, refusals and edge cases ----
def level_sizes(m):
    return [(s.x, s.y, s.z) for s in (m.level_domain(l).size() for l in range(m.levels))]


def case_levels(st, backend):
    def mg(size, **kw):
        return st.StarMG(size, poisson(), backend=backend, gpus=kw.pop("gpus", [0]), group=st.make_single_group(), **kw)

    assert level_sizes(mg((32, 32, 32))) == [(32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3]
    assert mg((32, 32, 32), gpus=[0, 0]).levels == 3
    assert level_sizes(mg((48, 32, 32), min_size=4)) == [(48, 32, 32), (24, 16, 16), (12, 8, 8), (6, 4, 4)]
    assert level_sizes(mg((30, 32, 32))) == [(30, 32, 32), (15, 16, 16)]
    assert mg((32, 32, 32), max_levels=2).levels == 2
    assert mg((32, 32, 32), min_size=8).levels == 3
    with pytest.raises(ValueError, match="31"):
        mg((31, 32, 32))
    with pytest.raises(ValueError, match="two levels"):
        mg((6, 32, 32))  # 3 < min_size
    op = conditions(None, None, (FC.open(), FC.mirror()))
    with pytest.raises(ValueError, match="Open"):
        mg((32, 32, 32), boundary=op)
    # a callable gives every level its weights
    seen = []
    m = mg((16, 16, 16), max_levels=3)
    m2 = st.StarMG((16, 16, 16), lambda l: (seen.append(l), m.level_weights(l))[1], backend=backend, gpus=[0],
                   group=st.make_single_group(), max_levels=3)
    assert seen == [0, 1, 2] and m2.levels == 3
    # s I + D / 4^l
    h = helmholtz(0.5)
    mh = st.StarMG((16, 16, 16), h, backend=backend, gpus=[0], group=st.make_single_group(), max_levels=3)
    for l in range(3):
        wl = mh.level_weights(l)
        assert abs(wl.center - (0.5 + 6.0 / 4 ** l)) < 1e-15 and wl.get(0, 0, 1) == -1.0 / 4 ** l, (l, wl.center)


def case_limits(st, backend):
    dtype = torch.float64
    f = rhs((16, 16, 16), dtype)
    m, _ = make_mg(st, backend, (16, 16, 16), poisson(), all_antimirror(), dtype, f=torch.zeros_like(f))
    m.set_guess(lambda gz, gy, gx: (gz + gy + gx).to(torch.float64))
    assert m.solve() == (0, 0.0) and not gather_solution(m).any() and m.history == []
    bad = f.clone()
    bad[3, 4, 5] = math.nan
    m, _ = make_mg(st, backend, (16, 16, 16), poisson(), all_antimirror(), dtype, f=bad)
    with pytest.raises(FloatingPointError):
        m.solve()
    # max_cycles caps the solve, and solving again continues from the current u
    m, _ = make_mg(st, backend, (16, 16, 16), poisson(), all_antimirror(), dtype)
    cycles, rel = m.solve(tol=1e-10, max_cycles=2)
    assert cycles == 2 and len(m.history) == 2 and 1e-10 <= rel < 0.35 ** 2, (cycles, rel)
    cycles2, rel2 = m.solve(tol=1e-10)
    assert rel2 < 1e-10 and m.history[0] < rel, (rel, m.history)
    assert m.solve(tol=1e-10, max_cycles=0) == (0, rel2)
