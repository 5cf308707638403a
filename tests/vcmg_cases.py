"""Cases shared by test_vcmg.py (host backend) and test_gpu_vcmg.py (the HIP kernels): the StarMG V-cycle solver on
the variable-coefficient operator sigma - div(kappa grad) (ops.operator_varcoef, ops.varcoef_relax).

One cycle is compared bitwise with ops.varcoef_mg_cycle_reference on the gathered grid. The convergence limits are the
ones mg_cases.py uses for constant coefficients (within 12 cycles to 1e-6, every factor of the first six cycles
<= 0.35). They come from a torch prototype of the same arithmetic (V(2,2), omega 6/7, 32 coarse sweeps, arithmetic-mean
restricted kappa), not from the code under test: its worst factors were 0.235 to 0.242 for the smooth coefficient and
0.268 to 0.279 for exp(0.5 randn), 9 and 10 cycles to 1e-6. For the fields committed here the oracle alone gives
first-five factors up to 0.243 (smooth, 9 cycles) and 0.283 (rough, 10 cycles), and 1e-5 in fp32 after 7 cycles. The
reference histories are computed once per case and shared.

A sharp jump is a documented limit, not a target: kappa = 1 + 9 (x >= 16) between AntiMirror walls raised the
prototype's factors to 0.39 (5e-6 after 10 cycles, 1e-6 after 12; the oracle on the field here: factors up to 0.43,
1e-5 after 10 cycles), so that case asserts only 1e-5 within 12 cycles and agreement with the oracle's history."""
import functools
import math

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (coarsened_weights, operator_varcoef, restrict_reference, smoother_weights, star_weights,
                              varcoef_mg_cycle_reference, varcoef_relax_reference, varcoef_to_lists, weights_center)

from algebra_cases import gather_solution, same_bits
from mg_cases import FC, conditions, cycle_walls, level_sizes, rhs
from varcoef_cases import global_kappa, mirror_twin

DTYPES = [torch.float64, torch.float32]
SIZE = (32, 32, 32)
NU, OMEGA, COARSE = (2, 2), 6.0 / 7.0, 32


# ---- coefficients ----
@functools.lru_cache(maxsize=None)
def kappa_field(kind, size, dtype):
    """"smooth": 1 + 0.5 sin cos + 0.25 sin at the cell centres, wavelengths that divide the extents (periodic cases);
    "rough": exp(0.5 randn), seeded; "jump": 1 + 9 (x >= X / 2); "unit": 0.5 + rand (varcoef_cases.global_kappa)"""
    X, Y, Z = size
    if kind == "unit":
        return global_kappa(size, dtype)
    if kind == "rough":
        g = torch.Generator().manual_seed(1201)
        return torch.exp(0.5 * torch.randn((Z, Y, X), generator=g, dtype=torch.float64)).to(dtype)
    z = (torch.arange(Z, dtype=torch.float64) + 0.5).view(-1, 1, 1)
    y = (torch.arange(Y, dtype=torch.float64) + 0.5).view(1, -1, 1)
    x = (torch.arange(X, dtype=torch.float64) + 0.5).view(1, 1, -1)
    if kind == "jump":
        return (1.0 + 9.0 * (x >= X / 2).double() + 0 * (y + z)).to(dtype)
    assert kind == "smooth", kind
    two_pi = 2 * math.pi
    k = 1 + 0.5 * torch.sin(two_pi * x / X) * torch.cos(two_pi * 2 * y / Y) + 0.25 * torch.sin(two_pi * 2 * z / Z)
    return k.to(dtype)


def walls(name):
    """"antimirror": AntiMirror(0) on every face; "periodic"; "mixed": AntiMirror x, Mirror y, periodic z"""
    if name == "periodic":
        return None
    if name == "antimirror":
        return conditions(*[(FC.antimirror(0.0), FC.antimirror(0.0))] * 3)
    assert name == "mixed", name
    return conditions((FC.antimirror(0.0), FC.antimirror(0.0)), (FC.mirror(), FC.mirror()), None)


# name -> (kappa kind, walls, sigma, gpus, levels); the periodic operator needs sigma > 0 to be regular
CONVERGENCE = {
    "smooth_antimirror": ("smooth", "antimirror", 0.0, (0,), 4),
    "smooth_antimirror_two": ("smooth", "antimirror", 0.0, (0, 0), 3),
    "smooth_periodic": ("smooth", "periodic", 0.01, (0,), 4),
    "smooth_mixed": ("smooth", "mixed", 0.0, (0,), 4),
    "rough_antimirror": ("rough", "antimirror", 0.0, (0,), 4),
    "rough_periodic": ("rough", "periodic", 0.01, (0,), 4),
    "rough_mixed": ("rough", "mixed", 0.0, (0,), 4),
}
JUMP = ("jump", "antimirror", 0.0, (0,), 4)


def kappa_fn(kappa):
    Z, Y, X = kappa.shape
    return lambda gz, gy, gx: kappa.to(gz.device)[gz % Z, gy % Y, gx % X]


def make_mg(st, backend, size, w, kappa, bc, dtype, gpus=(0,), f=None, group=None, methods=None, **kw):
    if methods is not None:
        kw["methods"] = methods
    m = st.StarMG(size, w, fp64=dtype == torch.float64, gpus=list(gpus), backend=backend, boundary=bc,
                  group=group if group is not None else st.make_single_group(), kappa=kappa_fn(kappa), **kw)
    f = rhs(size, dtype) if f is None else f
    m.set_rhs(kappa_fn(f))
    return m, f


def relres(u, f, kappa, w, bc, kbc=None):
    """||f - A u||2 / ||f||2: the residual in the fields' type as the solver forms it, the sums in float64"""
    if bc is not None and kbc is None:
        kbc = mirror_twin(bc)
    r = varcoef_relax_reference(u, kappa, f, w, boundary=bc, kappa_boundary=kbc).double()
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


def gather_kappa(m, l):
    dd = m.level_domain(l)
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=m.dtype)
    m.synchronize()
    for di in range(dd.num_domains()):
        o, s = dd.domain(di).origin(), dd.domain(di).size()
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = m.level_kappa(l, di).cpu()
    return out


# ---- 1. one cycle, bitwise ----
def cycle_reference(m, f, kappa, bc, u=None):
    ws = [m.level_weights(l) for l in range(m.levels)]
    return varcoef_mg_cycle_reference(torch.zeros_like(f) if u is None else u, f, kappa, ws, bc, None, m.nu, m.omega,
                                      m.coarse_sweeps)


def case_cycle(st, backend, dtype):
    size, w, bc = (16, 16, 16), operator_varcoef(0.0), cycle_walls()
    kappa = kappa_field("unit", size, dtype)
    m, f = make_mg(st, backend, size, w, kappa, bc, dtype, max_levels=3)
    assert m.levels == 3 and level_sizes(m) == [(16,) * 3, (8,) * 3, (4,) * 3]
    assert (m.u, m.f, m.r, m.kappa, m.v) == (0, 1, 2, 3, 4)
    want_k = kappa
    for l in range(m.levels):
        assert same_bits(gather_kappa(m, l), want_k), f"kappa of level {l}"
        want_k = restrict_reference(want_k)
    m.cycle()
    got = gather_solution(m)
    want = cycle_reference(m, f, kappa, bc)
    bad = int((got != want).sum())
    assert same_bits(got, want), f"{dtype}: {bad} cells differ, max {float((got - want).abs().max()):.3e}"
    rel = relres(got, f, kappa, w, bc)
    print(f"one cycle {dtype}: relres {rel:.3e}")
    assert rel < 0.35  # and it is a multigrid cycle, not only the same arithmetic


# ---- 2. convergence against the prototype's limits and the reference's history ----
def problem(case, dtype):
    kind, wall, sigma, gpus, levels = case
    return kappa_field(kind, SIZE, dtype), walls(wall), operator_varcoef(sigma), gpus, levels


@functools.lru_cache(maxsize=None)
def reference_history(case, dtype, cycles):
    """relres after each of `cycles` reference cycles (computed once per case)"""
    kappa, bc, w, _, levels = problem(case, dtype)
    ws = [coarsened_weights(w, l) for l in range(levels)]
    f = rhs(SIZE, dtype)
    u = torch.zeros_like(f)
    out = []
    for _ in range(cycles):
        u = varcoef_mg_cycle_reference(u, f, kappa, ws, bc, None, NU, OMEGA, COARSE)
        out.append(relres(u, f, kappa, w, bc))
    return tuple(out)


def _solve_and_compare(st, backend, case, dtype, tol, what):
    kappa, bc, w, gpus, levels = problem(case, dtype)
    m, f = make_mg(st, backend, SIZE, w, kappa, bc, dtype, gpus)
    assert m.levels == levels and m.domain.num_domains() == len(gpus), (m.levels, m.domain.num_domains())
    cycles, rel = m.solve(tol=tol)
    h = m.history
    factors = [h[k + 1] / h[k] for k in range(min(5, len(h) - 1))]
    print(f"{what}: cycles {cycles} relres {rel:.3e} history {['%.3e' % v for v in h]} factors {['%.3f' % v for v in factors]}")
    assert cycles == len(h) <= 12 and rel == h[-1] < tol, (cycles, h)
    true = relres(gather_solution(m), f, kappa, w, bc)
    assert abs(true - rel) <= 1e-6 * rel + 1e-14, (true, rel)
    ref = reference_history(case, dtype, cycles)
    for k, (a, b) in enumerate(zip(h, ref)):
        assert abs(a - b) <= 1e-6 * b, f"cycle {k + 1}: relres {a!r}, reference {b!r}"
    return factors


def case_convergence(st, backend, name):
    factors = _solve_and_compare(st, backend, CONVERGENCE[name], torch.float64, 1e-6, name)
    assert len(factors) == 5 and all(v <= 0.35 for v in factors), factors


def case_fp32(st, backend):
    kappa, bc, w, gpus, levels = problem(CONVERGENCE["smooth_antimirror"], torch.float32)
    m, f = make_mg(st, backend, SIZE, w, kappa, bc, torch.float32, gpus)
    cycles, rel = m.solve(tol=1e-5)
    print(f"fp32: cycles {cycles} relres {rel:.3e} history {['%.3e' % v for v in m.history]}")
    assert m.levels == levels and cycles <= 10 and rel < 1e-5, (cycles, m.history)


def case_jump(st, backend):
    """a contrast of 10 across x = 16: slower than the smooth cases (a documented limit), still 1e-5 within 12 cycles"""
    _solve_and_compare(st, backend, JUMP, torch.float64, 1e-5, "jump")


# ---- 3. the constructor, the level weights and edge cases ----
def case_levels(st, backend):
    one = lambda gz, gy, gx: 1.0 + 0 * (gz + gy + gx)  # noqa: E731
    kw = dict(backend=backend, gpus=[0], group=st.make_single_group())
    w = operator_varcoef(0.5)
    star = star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])
    with pytest.raises(ValueError, match="kappa"):
        st.StarMG((16, 16, 16), w, **kw)
    with pytest.raises(ValueError, match="kappa"):
        st.StarMG((16, 16, 16), star, kappa=one, **kw)
    mir = conditions(*[(FC.mirror(), FC.mirror())] * 3)
    with pytest.raises(ValueError, match="kappa"):
        st.StarMG((16, 16, 16), star, boundary=mir, kappa_boundary=mir, **kw)
    with pytest.raises(ValueError, match="kappa_boundary needs boundary"):
        st.StarMG((16, 16, 16), w, kappa=one, kappa_boundary=mir, **kw)
    for ax in range(3):
        faces = [None, None, None]
        faces[ax] = (FC.mirror(), FC.open())
        op = conditions(*faces)
        with pytest.raises(ValueError, match="Open"):
            st.StarMG((16, 16, 16), w, kappa=one, boundary=op, **kw)
        with pytest.raises(ValueError, match="Open"):
            st.StarMG((16, 16, 16), w, kappa=one, boundary=mir, kappa_boundary=op, **kw)
    with pytest.raises(ValueError, match="two levels"):
        st.StarMG((6, 32, 32), w, kappa=one, **kw)
    # shift kept, h / 4^level; a VarCoefWeights has no constant centre
    m = st.StarMG((16, 16, 16), w, kappa=one, max_levels=3, **kw)
    assert m.levels == 3
    for l in range(3):
        assert varcoef_to_lists(m.level_weights(l)) == (0.5, [-0.5 / 4 ** l] * 3), l
        assert varcoef_to_lists(coarsened_weights(w, l)) == (0.5, [-0.5 / 4 ** l] * 3), l
    with pytest.raises(TypeError, match="VarCoefWeights"):
        weights_center(w)
    with pytest.raises(TypeError, match="VarCoefWeights"):
        smoother_weights(w, 0.1)
    # a callable gives every level its weights
    seen = []
    m2 = st.StarMG((16, 16, 16), lambda l: (seen.append(l), m.level_weights(l))[1], kappa=one, max_levels=3, **kw)
    assert seen == [0, 1, 2] and m2.levels == 3
    assert varcoef_to_lists(m2.level_weights(2)) == varcoef_to_lists(m.level_weights(2))
    # star weights are unchanged: no coefficient, no second iterate
    ms = st.StarMG((16, 16, 16), star, max_levels=3, **kw)
    assert ms.kappa is None and ms.v is None
    with pytest.raises(ValueError, match="VarCoefWeights"):
        ms.set_kappa(one)


def case_limits(st, backend):
    dtype, size = torch.float64, (16, 16, 16)
    w, bc = operator_varcoef(0.0), walls("antimirror")
    kappa = kappa_field("unit", size, dtype)
    f = rhs(size, dtype)
    m, _ = make_mg(st, backend, size, w, kappa, bc, dtype, f=torch.zeros_like(f))
    m.set_guess(lambda gz, gy, gx: (gz + gy + gx).to(torch.float64))
    assert m.solve() == (0, 0.0) and not gather_solution(m).any() and m.history == []
    bad = f.clone()
    bad[3, 4, 5] = math.nan
    m, _ = make_mg(st, backend, size, w, kappa, bc, dtype, f=bad)
    with pytest.raises(FloatingPointError):
        m.solve()
    # max_cycles caps the solve, and solving again continues from the current u
    m, _ = make_mg(st, backend, size, w, kappa, bc, dtype)
    cycles, rel = m.solve(tol=1e-10, max_cycles=2)
    assert cycles == 2 and len(m.history) == 2 and 1e-10 <= rel < 0.35 ** 2, (cycles, rel)
    cycles2, rel2 = m.solve(tol=1e-10)
    assert rel2 < 1e-10 and m.history[0] < rel, (rel, m.history)
    assert m.solve(tol=1e-10, max_cycles=0) == (0, rel2)
    # an odd number of sweeps ends in u as well (one copy)
    m, _ = make_mg(st, backend, size, w, kappa, bc, dtype, nu=(1, 3), max_levels=3)
    m.cycle()
    assert same_bits(gather_solution(m), cycle_reference(m, f, kappa, bc))
    # set_kappa replaces the coefficient on every level: the next cycle is the other operator's
    m, _ = make_mg(st, backend, size, w, kappa, bc, dtype, max_levels=3)
    m.cycle()
    first = gather_solution(m)
    other = kappa_field("smooth", size, dtype)
    m.set_kappa(kappa_fn(other))
    assert same_bits(gather_kappa(m, 1), restrict_reference(other))
    m.cycle()
    assert same_bits(gather_solution(m), cycle_reference(m, f, other, bc, u=first))
    assert not same_bits(gather_solution(m), cycle_reference(m, f, kappa, bc, u=first))
