"""Conjugate gradients for A u = f, where A is the operator ``ops.star_apply`` computes from symmetric star weights
(or ``ops.box_apply`` from symmetric 27-point box weights, e.g. the compact Laplacians of ``ops.laplacian_box``) under
physical boundary conditions (periodic, or Constant / Mirror / AntiMirror walls).

``StarCG`` is a thin Python class over ``parallel.DistributedDomain`` with four quantities of one dtype, u, r, p and
f. Every product A p is exchange + ``apply_boundary(p)`` + ``star_apply(p)`` (into next(p)), every vector update is
``DistributedDomain.axpby`` (the residual update returns ||r||^2 from the same pass) and p.Ap is
``DistributedDomain.reduce``. u takes ``boundary``; p takes its homogeneous twin (the same kinds, every Constant /
AntiMirror value 0); r and f take Open faces. An inhomogeneous wall therefore enters once, through
r0 = f - A_bc(u0), and every later product is with the linear operator.

With ``VarCoefWeights`` (``ops.operator_varcoef``) and ``kappa=fn`` A is the variable-coefficient operator of
``ops.varcoef_apply``: a fifth quantity, kappa, is added after u, r, p and f, filled from ``fn`` and given its halos and
ghost cells once at construction (``kappa_boundary``; None = Mirror on every non-periodic face of ``boundary``). That
operator is symmetric by construction, so no symmetry check applies.

Singular operators (a periodic or all-Mirror Laplacian with no centre shift) are the caller's responsibility: f must
sum to zero, and the solver does no projection.
"""
from __future__ import annotations

import math

import torch

from .. import _C
from ..ops.kernels import (box_apply, box_supported, field_axpby_supported, star_apply, star_supported, varcoef_apply,
                           varcoef_supported)
from ..parallel.domain import DistributedDomain
from .varcoef_model import kappa_conditions, refuse_open

_AXES = ((0, (-1, 0, 0), (1, 0, 0)), (1, (0, -1, 0), (0, 1, 0)), (2, (0, 0, -1), (0, 0, 1)))


def _conditions(boundary, homogeneous: bool, all_open: bool = False):
    """`boundary` with every Constant / AntiMirror value 0 (homogeneous), or Open on every non-periodic face"""
    bc = _C.BoundaryConditions()
    for ax, lo, hi in _AXES:
        faces = []
        for d in (lo, hi):
            c = boundary.face(*d)
            if c.kind == _C.FaceKind.Periodic:
                faces.append(_C.FaceCondition.periodic())
            elif all_open:
                faces.append(_C.FaceCondition.open())
            elif homogeneous and c.kind == _C.FaceKind.Constant:
                faces.append(_C.FaceCondition.constant(0.0))
            elif homogeneous and c.kind == _C.FaceKind.AntiMirror:
                faces.append(_C.FaceCondition.antimirror(0.0))
            else:
                faces.append(c)
        bc.set_axis(ax, faces[0], faces[1])
    return bc


def _check_box_symmetry(weights, boundary):
    """A box gives a symmetric matrix when w(d) == w(-d) for all d and, for every non-periodic axis a, also
    w(d) == w(d reflected in a): under Mirror / AntiMirror walls central symmetry alone does not (the ghost cell of a
    wall row folds w(d) onto the reflected offset's column)."""
    offs = (-1, 0, 1)
    for dz in offs:
        for dy in offs:
            for dx in offs:
                if weights.get(dz, dy, dx) != weights.get(-dz, -dy, -dx):
                    raise ValueError(f"StarCG needs symmetric weights: offset (dz, dy, dx) = ({dz}, {dy}, {dx}): "
                                     f"{weights.get(dz, dy, dx)} != {weights.get(-dz, -dy, -dx)} at the opposite offset")
    if boundary is None:
        return
    for ax, lo, hi in _AXES:
        if all(boundary.face(*d).kind == _C.FaceKind.Periodic for d in (lo, hi)):
            continue
        for dz in offs:
            for dy in offs:
                for dx in offs:
                    r = [dz, dy, dx]
                    r[2 - ax] = -r[2 - ax]
                    if weights.get(dz, dy, dx) != weights.get(*r):
                        raise ValueError(f"StarCG needs weights even along the walled axis {ax}: offset (dz, dy, dx) = "
                                         f"({dz}, {dy}, {dx}): {weights.get(dz, dy, dx)} != {weights.get(*r)} at its "
                                         f"reflection")


class StarCG:
    def __init__(self, size, weights, fp64: bool = True, gpus=None, backend=None, methods=_C.MethodFlags.All,
                 group=None, boundary=None, kappa=None, kappa_boundary=None):
        self._box = isinstance(weights, _C.BoxWeights)
        self._varcoef = isinstance(weights, _C.VarCoefWeights)
        if self._varcoef and kappa is None:
            raise ValueError("StarCG on VarCoefWeights needs the coefficient: kappa=fn(gz, gy, gx)")
        if not self._varcoef and (kappa is not None or kappa_boundary is not None):
            raise ValueError(f"kappa= / kappa_boundary= belong to VarCoefWeights, not {type(weights).__name__}")
        if self._varcoef:
            # symmetric by construction: kappa(c) + kappa(n) is the same sum from both sides
            R = 1
            if boundary is None and kappa_boundary is not None:
                raise ValueError("kappa_boundary needs boundary: the periodic faces of u and kappa are the grid's")
            refuse_open(kappa_boundary, "StarCG (kappa)")
        elif self._box:
            R = 1
            _check_box_symmetry(weights, boundary)
        else:
            R = weights.radius
            if R not in (1, 2, 3):
                raise ValueError(f"star radius must be 1, 2 or 3, not {R}")
            for ax in range(3):
                for k in range(1, R + 1):
                    if weights.get(ax, 0, k) != weights.get(ax, 1, k):
                        raise ValueError(f"StarCG needs symmetric weights: axis {ax}, offset {k}: "
                                         f"{weights.get(ax, 0, k)} != {weights.get(ax, 1, k)}")
        if boundary is not None:
            for ax, lo, hi in _AXES:
                for d in (lo, hi):
                    if boundary.face(*d).kind == _C.FaceKind.Open:
                        raise ValueError(f"StarCG cannot take an Open face (axis {ax}): nothing defines the operator there")
        self.weights = weights
        self.boundary = boundary
        self.dtype = torch.float64 if fp64 else torch.float32
        dd = DistributedDomain(*size, group=group)
        # a star reads faces only, a box edges and corners too
        dd.set_radius(_C.Radius.face_edge_corner(1, 1, 1) if self._box else _C.Radius.face_edge_corner(R, 0, 0))
        dd.set_methods(methods)
        if gpus is not None:
            dd.set_gpus(list(gpus))
        if backend is not None:
            dd.set_backend(backend)
        self.u, self.r, self.p, self.f = (dd.add_data(n, self.dtype) for n in ("u", "r", "p", "f"))
        # the coefficient comes after u, r, p, f, so their indices are the same for every kind of weights
        self.kappa = dd.add_data("kappa", self.dtype) if self._varcoef else None
        more_open = tuple(self._add_quantities(dd))
        if boundary is not None:
            dd.set_boundary_conditions(boundary)
            dd.set_boundary_conditions(self.p, _conditions(boundary, True))
            for q in (self.r, self.f) + more_open:
                dd.set_boundary_conditions(q, _conditions(boundary, False, all_open=True))
            if self._varcoef:
                dd.set_boundary_conditions(self.kappa, kappa_conditions(boundary, kappa_boundary))
        dd.realize()
        for di in range(dd.num_domains()):
            if self._varcoef:
                ok = varcoef_supported(dd, di, self.u, self.kappa) and varcoef_supported(dd, di, self.p, self.kappa)
            else:
                ok = box_supported(dd, di, self.u) if self._box else star_supported(dd, di, self.u, weights)
            assert ok and field_axpby_supported(dd, di, self.r, self.f, self.u)
        self._dd = dd
        self._size = tuple(int(v) for v in size)
        if self._varcoef:
            # CG never swaps, so curr(kappa) is the coefficient for good: its halos and ghost cells are set once here
            # (the exchange inside every product re-sends the same values)
            dd.fill_from_global(self.kappa, kappa)
            dd.exchange()
            if boundary is not None:
                dd.apply_boundary(self.kappa)
        self.set_guess()

    def _add_quantities(self, dd):
        """a subclass adds its quantities here, after u, r, p, f (and kappa), and returns those that take Open faces"""
        return ()

    def _zero(self, gz, gy, gx):
        return torch.zeros((), dtype=self.dtype, device=gz.device) * (gz + gy + gx)

    def set_rhs(self, fn):
        """f = fn(gz, gy, gx) (torch index tensors of global coordinates, as StarStencil3D.init)"""
        self._dd.fill_from_global(self.f, fn)
        return self

    def set_guess(self, fn=None):
        """u0 = fn(gz, gy, gx); default 0"""
        self._dd.fill_from_global(self.u, fn if fn is not None else self._zero)
        return self

    def _apply(self, q):
        """next(q) = A curr(q) under q's boundary conditions"""
        dd = self._dd
        dd.exchange()  # blocking; orders itself after the null stream, where the kernels below run
        if self.boundary is not None:
            dd.apply_boundary(q)
        for di in range(dd.num_domains()):
            if self._varcoef:
                varcoef_apply(dd, di, q, self.kappa, self.weights)
            elif self._box:
                box_apply(dd, di, q, self.weights)
            else:
                star_apply(dd, di, q, self.weights)

    @staticmethod
    def _finite(s, what):
        if s.nonfinite > 0:
            raise FloatingPointError(f"StarCG: {s.nonfinite} non-finite cells in {what}")

    def solve(self, tol: float = 1e-8, max_iters: int = 1000):
        """Conjugate gradients from the current u until ||r||2 / ||f||2 < tol (r the recursively updated residual) or
        `max_iters` iterations: returns (iters, relres). alpha and beta are Python doubles, converted to the element
        type by the kernels. A negative-definite operator (a plain Laplacian) needs no special case: p.Ap and alpha
        are negative. Singular operators are the caller's responsibility (f must sum to zero; no projection is done).
        Raises FloatingPointError when a reduction sees a non-finite cell or p.Ap is 0 or not finite. f = 0 returns
        (0, 0.0) with u = 0. Collective: every reduction is, so all ranks compute the same alpha and beta and stop at
        the same iteration."""
        dd, u, r, p, f = self._dd, self.u, self.r, self.p, self.f
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
        dd.copy(p, r)
        it = 0
        while it < max_iters and math.sqrt(rr / ff) >= tol:
            self._apply(p)  # next(p) = A p
            pAp = dd.reduce(p, other=p, curr=True, other_curr=False).dot
            if pAp == 0 or not math.isfinite(pAp):
                raise FloatingPointError(f"StarCG: p.Ap = {pAp} at iteration {it}")
            alpha = rr / pAp
            dd.axpby(u, 1.0, u, alpha, p)
            s = dd.axpby(r, 1.0, r, -alpha, p, y_curr=False, stats=True)
            self._finite(s, f"the residual of iteration {it}")
            rr_new = s.sum_sq
            beta = rr_new / rr
            dd.axpby(p, 1.0, r, beta, p)
            rr = rr_new
            it += 1
        return it, math.sqrt(rr / ff)

    def synchronize(self):
        if self._dd.backend() == _C.Backend.Device and torch.cuda.is_available():
            torch.cuda.synchronize()

    @property
    def domain(self):
        return self._dd

    def cells(self) -> int:
        return self._size[0] * self._size[1] * self._size[2]

    def solution(self, di: int = 0) -> torch.Tensor:
        """interior (z, y, x) view of u on local sub-domain di"""
        return self._dd.interior(self._dd.curr(di, self.u), di)
