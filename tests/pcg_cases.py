"""Cases shared by test_pcg.py (host backend) and test_gpu_pcg.py (the HIP kernels): StarPCG, flexible conjugate
gradients preconditioned by one StarMG V-cycle, with the cycle in the outer type or in fp32 under an fp64 iteration.

apply_preconditioner is compared bitwise with convert_reference(cycle_reference(0, convert_reference(r, 1 / s)), s) on
the gathered grid, s being the solver's own norm (read back from precond_scale: the summation order of a reduction is
not pinned). The solves are compared with ops.mgpcg_reference on the same fields, never with another run of the code
under test.

The problem is -div(kappa grad u) = f with kappa = 1 + (c - 1) [x >= X / 2 and y >= Y / 4], f seeded normal deviates
(mean removed when every face is periodic). The absolute iteration caps (18 for c = 100, 25 for periodic c = 1000) come
from a torch prototype of the same arithmetic, which took 13 to 16 and 19 to 21 iterations to 1e-10; for the fields
committed here the oracle alone takes 13 (16^3 mixed, c = 100), 14 (32^3 AntiMirror, c = 100) and 19 (16^3 periodic,
c = 1000) with an fp64 cycle and the same counts with an fp32 cycle (test_pcg.py asserts that before anything else).

HISTORY_RTOL: the relres history of the fp64-preconditioned solve agrees with the oracle's within 1e-6 relative per
iteration, the margin vcmg_cases.py uses for cycles. It is not too tight for another summation order: with every dot
product of the oracle perturbed by one ulp (a random factor 1, 1 + 2^-52 or 1 - 2^-52, eight seeds) its own history
moved by at most 2e-13 (16^3 mixed), 1e-13 (32^3 AntiMirror) and 5.8e-8 (16^3 periodic, c = 1000) relative."""
import functools
import math

import pytest
import torch

from stencil2_amd import _C
from stencil2_amd.ops import (coarsened_weights, convert_reference, mg_cycle_reference, mgpcg_reference, operator_varcoef,
                              star_weights, varcoef_mg_cycle_reference, varcoef_step_reference)

from algebra_cases import gather_solution, same_bits
from mg_cases import FC, conditions, minus_box27, poisson
from reduce_cases import put, random_field
from varcoef_cases import mirror_twin

NU, OMEGA, COARSE = (2, 2), 6.0 / 7.0, 32
HISTORY_RTOL = 1e-6
F64, F32 = torch.float64, torch.float32


def walls(name):
    """"antimirror": AntiMirror(0) on every face; "periodic"; "mixed": Mirror on the low x face, AntiMirror(0) on the
    other five"""
    if name == "periodic":
        return None
    am = (FC.antimirror(0.0), FC.antimirror(0.0))
    if name == "antimirror":
        return conditions(am, am, am)
    assert name == "mixed", name
    return conditions((FC.mirror(), FC.antimirror(0.0)), am, am)


@functools.lru_cache(maxsize=None)
def kappa_field(size, c):
    X, Y, Z = size
    x = torch.arange(X).view(1, 1, -1)
    y = torch.arange(Y).view(1, -1, 1)
    z = torch.arange(Z).view(-1, 1, 1)
    return 1.0 + (c - 1.0) * ((x >= X // 2) & (y >= Y // 4) & (z >= 0)).double()


@functools.lru_cache(maxsize=None)
def rhs(size, periodic, seed=1301):
    X, Y, Z = size
    f = torch.randn((Z, Y, X), generator=torch.Generator().manual_seed(seed), dtype=F64)
    return f - f.mean() if periodic else f


def field_fn(t):
    Z, Y, X = t.shape
    return lambda gz, gy, gx: t.to(gz.device)[gz % Z, gy % Y, gx % X]


# name -> (size, walls, contrast, levels, iteration cap)
CONVERGENCE = {
    "mixed16_c100": ((16, 16, 16), "mixed", 100.0, 3, 18),
    "antimirror32_c100": ((32, 32, 32), "antimirror", 100.0, 4, 18),
    "periodic16_c1000": ((16, 16, 16), "periodic", 1000.0, 3, 25),
}
POINT = "antimirror32_c100"


def make_pcg(st, backend, size, w, bc, outer, precond, kappa=None, f=None, gpus=(0,), group=None, methods=None, **kw):
    if methods is not None:
        kw["methods"] = methods
    if kappa is not None:
        kw["kappa"] = field_fn(kappa)
    m = st.StarPCG(size, w, fp64=outer == F64, precond_fp64=precond == F64, boundary=bc, gpus=list(gpus),
                   backend=backend, group=group if group is not None else st.make_single_group(), **kw)
    if f is not None:
        m.set_rhs(field_fn(f))
    return m


def level_weights(w, levels):
    return [coarsened_weights(w, l) for l in range(levels)]


@functools.lru_cache(maxsize=None)
def oracle(name, outer, precond, tol, flexible=True, levels=None):
    """(iterations, history, u) of ops.mgpcg_reference for a convergence case (computed once, shared); `levels`
    other than the case's: a decomposition that stops coarsening earlier"""
    size, wall, c, case_levels, _ = CONVERGENCE[name]
    levels = case_levels if levels is None else levels
    w, bc = operator_varcoef(0.0), walls(wall)
    f = rhs(size, bc is None).to(outer)
    u, h = mgpcg_reference(torch.zeros_like(f), f, level_weights(w, levels), bc, kappa=kappa_field(size, c).to(outer),
                           precond_dtype=precond, nu=NU, omega=OMEGA, coarse_sweeps=COARSE, tol=tol, max_iters=200,
                           flexible=flexible)
    return len(h), tuple(h), u


def true_relres(u, f, kappa, w, bc):
    """||f - A u||2 / ||f||2 in float64 torch"""
    kbc = None if bc is None else mirror_twin(bc)
    r = f.double() - varcoef_step_reference(u.double(), kappa.double(), w, boundary=bc, kappa_boundary=kbc)
    return math.sqrt(float((r * r).sum()) / float((f.double() * f.double()).sum()))


# ---- 0. the caps hold for the oracle alone ----
def case_oracle_caps(name):
    cap = CONVERGENCE[name][4]
    for precond in (F64, F32):
        iters, h, _ = oracle(name, F64, precond, 1e-10)
        print(f"oracle {name} precond {precond}: {iters} iterations, last {h[-1]!r}")
        assert iters <= cap and h[-1] < 1e-10, (name, precond, iters, h)


# ---- 1. z = M r, bitwise ----
def gather(m, dd, q, dtype):
    g = dd.size()
    out = torch.empty((g.z, g.y, g.x), dtype=dtype)
    m.synchronize()
    for di in range(dd.num_domains()):
        o, s = dd.domain(di).origin(), dd.domain(di).size()
        out[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x] = dd.interior(dd.curr(di, q), di).cpu()
    return out


def case_preconditioner(st, backend, kind, outer, precond, gpus=(0,)):
    size = (16, 16, 16)
    if kind == "varcoef":
        w, bc, kappa = operator_varcoef(0.0), walls("mixed"), (0.5 + random_field(size, F64, 1311).abs()).to(outer)
    else:
        w, bc, kappa = star_weights(1, 6.01, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]), None, None
    m = make_pcg(st, backend, size, w, bc, outer, precond, kappa=kappa, gpus=gpus, max_levels=3)
    mg = m.preconditioner
    assert mg.levels == (3 if len(gpus) == 1 else 2) and m.domain.num_domains() == len(gpus) == mg.domain.num_domains()
    assert (m.u, m.r, m.p, m.f) == (0, 1, 2, 3) and m.z == (5 if kind == "varcoef" else 4)
    assert m.dtype == outer and mg.dtype == precond
    r = (1e3 * random_field(size, F64, 1312)).to(outer)  # a norm far from 1: the scaling matters
    put(m.domain, m.r, True, r)
    m.apply_preconditioner()
    s = m.precond_scale
    assert abs(s - float(r.double().norm())) <= 1e-12 * s, (s, float(r.double().norm()))
    got = gather(m, m.domain, m.z, outer)
    ws = [mg.level_weights(l) for l in range(mg.levels)]
    g = convert_reference(r, 1.0 / s, precond)
    if kind == "varcoef":
        kp = convert_reference(kappa, 1.0, precond)
        assert same_bits(gather(m, mg.domain, mg.kappa, precond), kp), "the cycle's coefficient is the rounded outer one"
        e = varcoef_mg_cycle_reference(torch.zeros_like(g), g, kp, ws, bc, None, NU, OMEGA, COARSE)
    else:
        e = mg_cycle_reference(torch.zeros_like(g), g, ws, bc, NU, OMEGA, COARSE)
    want = convert_reference(e, s, outer)
    bad = int((got != want).sum())
    assert same_bits(got, want), f"{kind} {outer} {precond}: {bad} cells differ, max {float((got - want).abs().max()):.3e}"
    assert same_bits(gather(m, m.domain, m.r, outer), r)  # r is read only


# ---- 2. convergence against the oracle ----
def case_convergence(st, backend, name, precond, gpus=(0,)):
    size, wall, c, levels, cap = CONVERGENCE[name]
    w, bc = operator_varcoef(0.0), walls(wall)
    kappa, f = kappa_field(size, c), rhs(size, bc is None)
    m = make_pcg(st, backend, size, w, bc, F64, precond, kappa=kappa, f=f, gpus=gpus)
    if len(gpus) == 2:
        levels -= 1  # halves of the grid coarsen once less
    assert m.preconditioner.levels == levels and m.domain.num_domains() == len(gpus)
    iters, rel = m.solve(tol=1e-10, max_iters=200)
    want_iters, want_h, _ = oracle(name, F64, precond, 1e-10, levels=levels)
    true_dev = m.true_residual()
    true = true_relres(gather_solution(m), f, kappa, w, bc)
    h = m.history
    print(f"{name} precond {precond}: iters {iters} (oracle {want_iters}) relres {rel:.3e} true {true:.3e} "
          f"(device {true_dev:.3e}) history {['%.3e' % v for v in h]}")
    print(f"  worst history deviation {max(abs(a - b) / b for a, b in zip(h, want_h)):.3e}")
    assert iters == len(h) and rel == h[-1] < 1e-10, (iters, rel, h)
    assert abs(iters - want_iters) <= 1, (iters, want_iters)
    if precond == F64:
        for k, (a, b) in enumerate(zip(h, want_h)):
            assert abs(a - b) <= HISTORY_RTOL * b, f"iteration {k + 1}: relres {a!r}, oracle {b!r}"
    assert true < 1e-10 and rel / 2 <= true <= 2 * rel, (true, rel)
    assert abs(true_dev - true) <= 1e-3 * true, (true_dev, true)
    assert iters <= cap, (iters, cap)
    return m


# ---- 3. the point of the feature ----
def case_point(st, backend):
    size, wall, c, levels, cap = CONVERGENCE[POINT]
    w, bc = operator_varcoef(0.0), walls(wall)
    kappa, f = kappa_field(size, c), rhs(size, False)
    kw = dict(gpus=[0], backend=backend, boundary=bc)
    m = make_pcg(st, backend, size, w, bc, F64, F32, kappa=kappa, f=f)
    iters, rel = m.solve(tol=1e-10)
    assert rel < 1e-10 and iters <= cap, (iters, rel)
    mg = st.StarMG(size, w, fp64=False, group=st.make_single_group(), kappa=field_fn(kappa), **kw)
    mg.set_rhs(field_fn(f))
    cycles, mrel = mg.solve(tol=1e-10, max_cycles=30)
    cg = st.StarCG(size, w, fp64=True, group=st.make_single_group(), kappa=field_fn(kappa), **kw)
    cg.set_rhs(field_fn(f))
    cit, crel = cg.solve(tol=1e-10, max_iters=300)
    print(f"StarPCG fp64 / fp32 cycle: {iters} iterations to {rel:.3e}; fp32 StarMG: {cycles} cycles to {mrel:.3e}; "
          f"fp64 StarCG: {cit} iterations to {crel:.3e}")
    assert cycles == 30 and mrel >= 1e-8, (cycles, mrel)
    assert cit == 300 and crel >= 1e-10 and 10 * iters < 300, (cit, crel, iters)


# ---- 4. options ----
def case_fp32(st, backend, name):
    size, wall, c, levels, cap = CONVERGENCE[name]
    w, bc = operator_varcoef(0.0), walls(wall)
    m = make_pcg(st, backend, size, w, bc, F32, F32, kappa=kappa_field(size, c), f=rhs(size, bc is None))
    iters, rel = m.solve(tol=1e-5)
    print(f"fp32 {name}: {iters} iterations, relres {rel:.3e}")
    assert rel < 1e-5 and iters <= cap, (iters, rel)


def case_not_flexible(st, backend):
    """beta = rho / rho_old runs and matches the oracle called with flexible=False, for c = 1"""
    size, w, bc = (16, 16, 16), operator_varcoef(0.0), walls("mixed")
    kappa, f = kappa_field(size, 1.0), rhs(size, False)
    m = make_pcg(st, backend, size, w, bc, F64, F64, kappa=kappa, f=f, flexible=False)
    iters, rel = m.solve(tol=1e-10)
    _, h = mgpcg_reference(torch.zeros_like(f), f, level_weights(w, 3), bc, kappa=kappa, nu=NU, omega=OMEGA,
                           coarse_sweeps=COARSE, tol=1e-10, flexible=False)
    print(f"flexible=False: {iters} iterations (oracle {len(h)}), relres {rel:.3e}")
    assert rel < 1e-10 and abs(iters - len(h)) <= 1, (iters, len(h))
    for k, (a, b) in enumerate(zip(m.history, h)):
        assert abs(a - b) <= HISTORY_RTOL * b, f"iteration {k + 1}: relres {a!r}, oracle {b!r}"


def case_constant_coefficients(st, backend, box):
    """star and box weights between AntiMirror walls: the prototype's c = 1 counts (9 and 10) + 2"""
    size, bc = (32, 32, 32), walls("antimirror")
    w = minus_box27() if box else poisson()
    f = rhs(size, False)
    m = make_pcg(st, backend, size, w, bc, F64, F32, f=f)
    iters, rel = m.solve(tol=1e-10)
    _, h = mgpcg_reference(torch.zeros_like(f), f, level_weights(w, 4), bc, precond_dtype=F32, nu=NU, omega=OMEGA,
                           coarse_sweeps=COARSE, tol=1e-10)
    print(f"box={box}: {iters} iterations (oracle {len(h)}), relres {rel:.3e}")
    assert rel < 1e-10 and iters <= (10 if box else 9) + 2 and abs(iters - len(h)) <= 1, (iters, len(h), rel)


def case_limits(st, backend):
    size, w, bc = (16, 16, 16), operator_varcoef(0.0), walls("mixed")
    kappa, f = kappa_field(size, 100.0), rhs(size, False)
    kw = dict(kappa=kappa)
    m = make_pcg(st, backend, size, w, bc, F64, F32, f=torch.zeros_like(f), **kw)
    m.set_guess(lambda gz, gy, gx: (gz + gy + gx).to(F64))
    assert m.solve() == (0, 0.0) and not gather_solution(m).any() and m.history == []
    bad = f.clone()
    bad[3, 4, 5] = math.nan
    m = make_pcg(st, backend, size, w, bc, F64, F32, f=bad, **kw)
    with pytest.raises(FloatingPointError):
        m.solve()
    # max_iters caps the solve, and solving again continues from the current u
    m = make_pcg(st, backend, size, w, bc, F64, F32, f=f, **kw)
    assert m.solve(tol=1e-10, max_iters=0) == (0, 1.0)
    iters, rel = m.solve(tol=1e-10, max_iters=3)
    assert iters == 3 and len(m.history) == 3 and 1e-10 <= rel < 1.0, (iters, rel)
    iters2, rel2 = m.solve(tol=1e-10)
    assert rel2 < 1e-10 and m.history[0] < rel and iters2 <= CONVERGENCE["mixed16_c100"][4], (iters2, rel2, m.history)
    assert true_relres(gather_solution(m), f, kappa, w, bc) < 1e-10
    single = dict(backend=backend, gpus=[0], group=st.make_single_group())
    with pytest.raises(ValueError, match="symmetric"):
        st.StarPCG(size, star_weights(1, 7.0, [-1.0, -1.5], [-1.0, -1.0], [-1.0, -1.0]), **single)
    op = conditions(None, None, (FC.open(), FC.mirror()))
    with pytest.raises(ValueError, match="Open"):
        st.StarPCG(size, poisson(), boundary=op, **single)
    with pytest.raises(ValueError, match="kappa"):
        st.StarPCG(size, w, **single)


def hexline(iters, rel):
    return f"pcg iters {iters} relres {float(rel).hex()}"
