"""Conjugate gradients preconditioned by one multigrid V-cycle, for the operators of ``StarCG``: symmetric star or
27-point box weights, or ``VarCoefWeights`` with ``kappa=fn``, under periodic faces or Constant / Mirror / AntiMirror
walls (no Open face).

``StarPCG`` is ``StarCG`` with a fifth field quantity z (after u, r, p, f and kappa, whose indices stay) and a
``StarMG`` built from the same size, weights, walls, GPUs, group and backend under the homogeneous twin of
``boundary``. The two solvers may differ in element type: ``fp64`` chooses the outer iteration's, ``precond_fp64`` the
cycle's (None: the outer one). An fp64 outer iteration with an fp32 cycle gives fp64 answers at the price of fp32
V-cycles.

z = M r is ``apply_preconditioner``: with s = ||r||2 (known from the residual update's fused stats)
``MG.f <- convert(r, 1 / s)``, ``MG.u <- 0``, one ``MG.cycle()``, ``z <- convert(MG.u, s)``, the two conversions being
``DistributedDomain.convert_from`` (``ops.field_convert``; with one type on both sides it is the cross-domain copy).
Scaling by 1 / s keeps the cycle's range independent of the magnitude of f. For ``VarCoefWeights`` the cycle's
coefficient is ``field_convert`` of the outer one, so an fp32 cycle sees exactly the rounded fp64 coefficient.

The cycle is not a symmetric operator (its restriction is the 8-cell mean, its prolongation trilinear), so the default
is the flexible (Polak-Ribiere) beta = z . (r - r_old) / rho_old = -alpha (z . Ap) / rho_old, which costs one more
reduction per iteration. ``flexible=False`` is the textbook beta = rho / rho_old; it is valid only for a symmetric
preconditioner, which this cycle is not, and can stall at high contrast.

Not provided: a symmetric (transposed) restriction, per-quantity exchange (the cycle's level-0 exchanges move all of
``StarMG``'s quantities), capture of the cycle in a hipGraph, fp16 / bf16. Singular operators are the caller's
responsibility, as in ``StarCG``.
"""
from __future__ import annotations

import math

from ..ops.kernels import field_convert_supported
from .multigrid import StarMG
from .star_cg import StarCG, _conditions


class StarPCG(StarCG):
    def __init__(self, size, weights, fp64: bool = True, precond_fp64=False, boundary=None, kappa=None,
                 kappa_boundary=None, nu=(2, 2), omega: float = 6.0 / 7.0, coarse_sweeps: int = 32, max_levels=None,
                 min_size: int = 4, flexible: bool = True, gpus=None, backend=None, methods=None, group=None):
        kw = {} if methods is None else dict(methods=methods)
        super().__init__(size, weights, fp64=fp64, gpus=gpus, backend=backend, group=group, boundary=boundary,
                         kappa=kappa, kappa_boundary=kappa_boundary, **kw)
        self.flexible = bool(flexible)
        self.history = []
        self.precond_scale = None
        pf = bool(fp64) if precond_fp64 is None else bool(precond_fp64)
        # the cycle corrects: every wall of its level 0 is homogeneous, whatever values `boundary` carries
        hom = None if boundary is None else _conditions(boundary, True)
        self._mg = StarMG(size, weights, fp64=pf, gpus=gpus, backend=backend, group=group, boundary=hom, nu=nu,
                          omega=omega, coarse_sweeps=coarse_sweeps, max_levels=max_levels, min_size=min_size, kappa=kappa,
                          kappa_boundary=kappa_boundary, **kw)
        self._check_partition()
        if self._varcoef:
            self._mg.domain.convert_from(self._dd, self._mg.kappa, self.kappa)
            self._mg._coarsen_kappa()

    def _add_quantities(self, dd):
        self.z = dd.add_data("z", self.dtype)
        return (self.z,)

    def _check_partition(self):
        dd, mdd = self._dd, self._mg.domain
        if dd.num_domains() != mdd.num_domains():
            raise RuntimeError(f"StarPCG: the preconditioner has {mdd.num_domains()} local sub-domains, the outer "
                               f"iteration {dd.num_domains()}")
        for di in range(dd.num_domains()):
            a, b = dd.domain(di), mdd.domain(di)
            same = (a.origin() == b.origin() and a.size() == b.size() and a.gpu() == b.gpu()
                    and field_convert_supported(dd, mdd, di, self.r, self._mg.f)
                    and field_convert_supported(mdd, dd, di, self._mg.u, self.z))
            if not same:
                raise RuntimeError(f"StarPCG: sub-domain {di} of the preconditioner ({b.get_compute_region()}, device "
                                   f"{b.gpu()}) is not the outer iteration's ({a.get_compute_region()}, device {a.gpu()})")

    @property
    def preconditioner(self) -> StarMG:
        return self._mg

    @staticmethod
    def _finite(s, what):
        if s.nonfinite > 0:
            raise FloatingPointError(f"StarPCG: {s.nonfinite} non-finite cells in {what}")

    def apply_preconditioner(self, s=None):
        """z = M r for the current r: one V-cycle from 0 on r / s, scaled back by s. `s` is ||r||2 (None: reduced
        here; collective); it is kept in `precond_scale`. Raises FloatingPointError when s is 0 or not finite."""
        dd, mg = self._dd, self._mg
        if s is None:
            st = dd.reduce(self.r)
            self._finite(st, "r")
            s = math.sqrt(st.sum_sq)
        if s == 0 or not math.isfinite(s):
            raise FloatingPointError(f"StarPCG: ||r|| = {s} cannot scale the preconditioner's right-hand side")
        self.precond_scale = s
        mdd = mg.domain
        mdd.convert_from(dd, mg.f, self.r, scale=1.0 / s)
        mg._zero(0, mg.u)
        mg.cycle()
        dd.convert_from(mdd, self.z, mg.u, scale=s)

    def true_residual(self) -> float:
        """||f - A u||2 / ||f||2 for the current u, formed in the outer type (into next(z)); collective"""
        dd = self._dd
        ff = dd.reduce(self.f).sum_sq
        self._apply(self.u)
        s = dd.axpby(self.z, 1.0, self.f, -1.0, self.u, dst_curr=False, y_curr=False, stats=True)
        return math.sqrt(s.sum_sq / ff) if ff > 0 else math.sqrt(s.sum_sq)

    def solve(self, tol: float = 1e-8, max_iters: int = 200):
        """Preconditioned conjugate gradients from the current u until ||r||2 / ||f||2 < tol (r the recursively
        updated residual) or `max_iters` iterations: returns (iters, relres); `history` holds the relres after every
        iteration. alpha and beta are Python doubles. Raises FloatingPointError when a reduction sees a non-finite
        cell, when p.Ap is 0 or not finite or when rho = r.z is 0. f = 0 returns (0, 0.0) with u = 0. Collective:
        every rank computes the same scalars and stops at the same iteration. Singular operators are the caller's
        responsibility (f must sum to zero; no projection is done)."""
        dd, u, r, p, f, z = self._dd, self.u, self.r, self.p, self.f, self.z
        self.history = []
        sf = dd.reduce(f)
        self._finite(sf, "f")
        ff = sf.sum_sq
        if ff == 0:
            self.set_guess()  # an exact 0 whatever u held
            return 0, 0.0
        self._apply(u)  # next(u) = A u0
        s = dd.axpby(r, 1.0, f, -1.0, u, y_curr=False, stats=True)
        self._finite(s, "the initial residual")
        rr = s.sum_sq
        it = 0
        if max_iters <= 0 or rr == 0 or math.sqrt(rr / ff) < tol:
            return it, math.sqrt(rr / ff)
        self.apply_preconditioner(math.sqrt(rr))
        rho = self._rho(it)
        dd.copy(p, z)
        while True:
            self._apply(p)  # next(p) = A p
            pAp = dd.reduce(p, other=p, curr=True, other_curr=False).dot
            if pAp == 0 or not math.isfinite(pAp):
                raise FloatingPointError(f"StarPCG: p.Ap = {pAp} at iteration {it}")
            alpha = rho / pAp
            dd.axpby(u, 1.0, u, alpha, p)
            s = dd.axpby(r, 1.0, r, -alpha, p, y_curr=False, stats=True)
            self._finite(s, f"the residual of iteration {it}")
            rr = s.sum_sq
            it += 1
            self.history.append(math.sqrt(rr / ff))
            if it >= max_iters or rr == 0 or self.history[-1] < tol:
                return it, self.history[-1]
            self.apply_preconditioner(math.sqrt(rr))
            rho_new = self._rho(it)
            if self.flexible:
                # z . (r - r_old) = -alpha z . Ap: next(p) still holds A p
                tau = dd.reduce(z, other=p, curr=True, other_curr=False).dot
                beta = -alpha * tau / rho
            else:
                beta = rho_new / rho
            dd.axpby(p, 1.0, z, beta, p)
            rho = rho_new

    def _rho(self, it):
        s = self._dd.reduce(self.r, other=self.z, curr=True, other_curr=True)
        rho = s.dot
        if rho == 0 or not math.isfinite(rho):
            raise FloatingPointError(f"StarPCG: r.z = {rho} at iteration {it}")
        return rho
