"""Geometric multigrid for A u = f, where A is the operator ``ops.star_apply`` computes from star weights (or
``ops.box_apply`` from 27-point box weights) under physical boundary conditions (periodic, or Constant / Mirror /
AntiMirror walls). The weights need not be symmetric.

``StarMG`` is a thin Python class over one ``parallel.DistributedDomain`` per level, each with three quantities of one
dtype, u, f and r. Level 0 is the caller's grid; level l + 1 has half the cells per axis (cell-centred coarsening, so
the walls of every level sit where the finest grid's do). A V(nu1, nu2) cycle smooths with damped Jacobi
(``ops.star_apply`` / ``ops.box_apply`` with the weights I - c A, then ``DistributedDomain.axpby``), restricts the
residual with ``ops.restrict_apply`` and corrects with ``ops.prolong_apply`` (u <- u + P e in one pass). u of level 0
takes ``boundary``; u of the coarser levels holds corrections and takes its homogeneous twin (the same kinds, every
Constant / AntiMirror value 0); r and f take Open faces.

Given one weights object A = s I + D (s the sum of all weights, the zeroth-order term), level l uses s I + D / 4^l:
the re-discretization at spacing 2^l h of a Laplacian, Helmholtz or implicit-diffusion operator. For any other
operator pass a callable ``level -> weights``.

The levels are decided from numbers every rank knows (the global size and the partition of level 0), and every level
is partitioned over the same GPUs; there is no agglomeration of coarse levels onto fewer GPUs, so a decomposition
into thin slabs stops coarsening early and leans on ``coarse_sweeps``.

With ``VarCoefWeights`` (``ops.operator_varcoef``) and ``kappa=fn`` A is the variable-coefficient operator of
``ops.varcoef_apply``, whose diagonal differs per cell. Every level then has two more quantities after u, f and r: the
coefficient kappa and a second iterate v with u's conditions. Level 0's kappa is ``fn``, level l + 1's the 8-cell mean
(``ops.restrict_apply``) of level l's, each given its halos and ghost cells once (``kappa_boundary``; None = Mirror on
every non-periodic face of ``boundary``). A smoothing sweep is the halo fill and one ``ops.varcoef_relax`` launch per
sub-domain (u + omega (f - A u) / diag(A) in one pass over u, kappa and f), sweeps alternating between u and v; the
residual is the same kernel in residual mode, its norm ``DistributedDomain.reduce``. Level l uses shift and h / 4^l.
Arithmetic-mean coarse coefficients keep the cycle's factor near the constant-coefficient one for smooth kappa and
moderate random kappa; sharp jumps slow it down (harmonic or Galerkin coarse operators are not provided), and
``StarCG`` remains the robust choice there.

Singular operators (a periodic or all-Mirror Laplacian with no centre shift) are the caller's responsibility, as in
``StarCG``.
"""
from __future__ import annotations

import math

import torch

from .. import _C
from ..ops.kernels import (box_apply, box_supported, field_axpby_supported, grid_transfer_supported, prolong_apply,
                           restrict_apply, star_apply, star_supported, varcoef_relax, varcoef_relax_supported)
from ..ops.multigrid import coarsened_weights, smoother_weights, weights_center
from ..parallel.domain import DistributedDomain
from .star_cg import _AXES, _conditions
from .varcoef_model import kappa_conditions, refuse_open


def plan_levels(size, dim, R: int, min_size: int = 4, max_levels=None):
    """(sizes, reason): the global size of every level for a grid of `size` partitioned into `dim` sub-domains per
    axis, and why coarsening stopped. Level l + 1 exists while every axis extent of level l is divisible by 2 x its
    partition dimension and the coarser sub-domain extents stay >= max(min_size, R), up to `max_levels`."""
    sizes = [tuple(int(v) for v in size)]
    floor = max(int(min_size), int(R))
    while True:
        if max_levels is not None and len(sizes) >= max_levels:
            return sizes, f"max_levels = {max_levels}"
        cur = sizes[-1]
        for ax in range(3):
            if cur[ax] % (2 * dim[ax]) != 0:
                return sizes, (f"extent {cur[ax]} of axis {ax} (level {len(sizes) - 1}) is not divisible by "
                               f"2 x {dim[ax]} sub-domains")
        for ax in range(3):
            if cur[ax] // 2 // dim[ax] < floor:
                return sizes, (f"extent {cur[ax]} of axis {ax} (level {len(sizes) - 1}) would leave sub-domains of "
                               f"{cur[ax] // 2 // dim[ax]} < {floor} cells")
        sizes.append(tuple(v // 2 for v in cur))


class StarMG:
    def __init__(self, size, weights, fp64: bool = True, gpus=None, backend=None, methods=_C.MethodFlags.All,
                 group=None, boundary=None, nu=(2, 2), omega: float = 6.0 / 7.0, coarse_sweeps: int = 32,
                 max_levels=None, min_size: int = 4, kappa=None, kappa_boundary=None):
        w0 = weights(0) if callable(weights) else weights
        self._box = isinstance(w0, _C.BoxWeights)
        self._varcoef = isinstance(w0, _C.VarCoefWeights)
        if self._varcoef and kappa is None:
            raise ValueError("StarMG on VarCoefWeights needs the coefficient: kappa=fn(gz, gy, gx)")
        if not self._varcoef and (kappa is not None or kappa_boundary is not None):
            raise ValueError(f"kappa= / kappa_boundary= belong to VarCoefWeights, not {type(w0).__name__}")
        if self._varcoef:
            if boundary is None and kappa_boundary is not None:
                raise ValueError("kappa_boundary needs boundary: the periodic faces of u and kappa are the grid's")
            refuse_open(kappa_boundary, "StarMG (kappa)")
        R = 1 if self._box or self._varcoef else w0.radius
        if R not in (1, 2, 3):
            raise ValueError(f"star radius must be 1, 2 or 3, not {R}")
        if boundary is not None:
            for ax, lo, hi in _AXES:
                for d in (lo, hi):
                    if boundary.face(*d).kind == _C.FaceKind.Open:
                        raise ValueError(f"StarMG cannot take an Open face (axis {ax}): nothing defines the operator there")
        if max_levels is not None and max_levels < 2:
            raise ValueError(f"StarMG needs at least two levels, max_levels = {max_levels}")
        self.boundary = boundary
        self.kappa_boundary = kappa_conditions(boundary, kappa_boundary) if self._varcoef else None
        self.kappa = self.v = None
        self.dtype = torch.float64 if fp64 else torch.float32
        self.nu = (int(nu[0]), int(nu[1]))
        self.omega = float(omega)
        self.coarse_sweeps = int(coarse_sweeps)
        self._R = R
        self._size = tuple(int(v) for v in size)
        self._cfg = dict(gpus=gpus, backend=backend, methods=methods, group=group)
        # the level rule needs the partition of level 0, which only its realize() decides: level 0 is realized
        # (collectively) before a grid that cannot coarsen is refused
        self._dds = [self._make_level(self._size, 0)]
        dim = self._dds[0].placement_dim()
        sizes, reason = plan_levels(self._size, (dim.x, dim.y, dim.z), R, min_size, max_levels)
        if len(sizes) < 2:
            raise ValueError(f"StarMG needs at least two levels: {reason}")
        self._stop = reason
        for l in range(1, len(sizes)):
            self._dds.append(self._make_level(sizes[l], l))
            self._check_pair(l)
        self._weights = [w0] + [weights(l) if callable(weights) else coarsened_weights(weights, l)
                                for l in range(1, len(sizes))]
        self._c, self._smoother = [], []
        for l, w in enumerate(self._weights):
            if self._varcoef or isinstance(w, _C.VarCoefWeights):
                if not (self._varcoef and isinstance(w, _C.VarCoefWeights)):
                    raise ValueError(f"the weights of level {l} differ in kind or radius from level 0")
                dd = self._dds[l]
                for di in range(dd.num_domains()):
                    assert all(varcoef_relax_supported(dd, di, self.u, self.kappa, self.f, q)
                               for q in (self.v, self.u, self.r))
                continue
            if isinstance(w, _C.BoxWeights) != self._box or (not self._box and w.radius != R):
                raise ValueError(f"the weights of level {l} differ in kind or radius from level 0")
            c = self.omega / weights_center(w)
            self._c.append(c)
            self._smoother.append(smoother_weights(w, c))
            dd = self._dds[l]
            for di in range(dd.num_domains()):
                ok = box_supported(dd, di, self.u) if self._box else star_supported(dd, di, self.u, w)
                assert ok and field_axpby_supported(dd, di, self.r, self.f, self.u)
        self.history = []
        for l in range(len(sizes)):
            for q in (self.u, self.f, self.r) + ((self.v,) if self._varcoef else ()):
                self._zero(l, q)
        self.synchronize()
        if self._varcoef:
            self.set_kappa(kappa)

    # ---- levels ----
    def _make_level(self, size, level):
        cfg = self._cfg
        dd = DistributedDomain(*size, group=cfg["group"])
        # a star reads faces only, a box and the prolongation edges and corners too
        dd.set_radius(_C.Radius.face_edge_corner(max(self._R, 1), 1, 1))
        dd.set_methods(cfg["methods"])
        if cfg["gpus"] is not None:
            dd.set_gpus(list(cfg["gpus"]))
        if cfg["backend"] is not None:
            dd.set_backend(cfg["backend"])
        self.u, self.f, self.r = (dd.add_data(n, self.dtype) for n in ("u", "f", "r"))
        if self._varcoef:
            # after u, f and r, whose indices are the same for every kind of weights
            self.kappa, self.v = (dd.add_data(n, self.dtype) for n in ("kappa", "v"))
        if self.boundary is not None:
            # the default conditions: u, and the second iterate v
            dd.set_boundary_conditions(self.boundary if level == 0 else _conditions(self.boundary, True))
            for q in (self.r, self.f):
                dd.set_boundary_conditions(q, _conditions(self.boundary, False, all_open=True))
            if self._varcoef:
                dd.set_boundary_conditions(self.kappa, self.kappa_boundary)
        dd.realize()
        return dd

    def _check_pair(self, l):
        fine, coarse = self._dds[l - 1], self._dds[l]
        if fine.num_domains() != coarse.num_domains():
            raise RuntimeError(f"StarMG: level {l} has {coarse.num_domains()} local sub-domains, level {l - 1} has "
                               f"{fine.num_domains()}")
        for di in range(fine.num_domains()):
            if not grid_transfer_supported(fine, coarse, di, self.u, self.u):
                raise RuntimeError(f"StarMG: sub-domain {di} of level {l} "
                                   f"({coarse.domain(di).get_compute_region()}, device {coarse.domain(di).gpu()}) is not "
                                   f"the factor-2 image of its parent ({fine.domain(di).get_compute_region()}, device "
                                   f"{fine.domain(di).gpu()})")

    @property
    def levels(self) -> int:
        return len(self._dds)

    def level_domain(self, l: int) -> DistributedDomain:
        return self._dds[l]

    def level_weights(self, l: int):
        return self._weights[l]

    @property
    def domain(self):
        return self._dds[0]

    def cells(self) -> int:
        return self._size[0] * self._size[1] * self._size[2]

    # ---- data ----
    def _zero(self, l, q):
        dd = self._dds[l]
        for di in range(dd.num_domains()):
            dd.curr(di, q).zero_()

    def set_rhs(self, fn):
        """f = fn(gz, gy, gx) (torch index tensors of global coordinates, as StarStencil3D.init)"""
        self._dds[0].fill_from_global(self.f, fn)
        return self

    def set_kappa(self, fn):
        """kappa = fn(gz, gy, gx) at level 0 and its 8-cell means on the coarser levels, then every level's halos and
        ghost cells of kappa, once: no kernel of the cycle writes curr(kappa) (VarCoefWeights only)"""
        if not self._varcoef:
            raise ValueError("set_kappa belongs to VarCoefWeights")
        self._dds[0].fill_from_global(self.kappa, fn)
        return self._coarsen_kappa()

    def _coarsen_kappa(self):
        """level 0's kappa is set: the coarser levels' means, then every level's halos and ghost cells"""
        for l in range(1, self.levels):
            fine, coarse = self._dds[l - 1], self._dds[l]
            for di in range(fine.num_domains()):
                restrict_apply(fine, coarse, di, self.kappa, self.kappa)
        for dd in self._dds:
            dd.exchange()
            if self.boundary is not None:
                dd.apply_boundary(self.kappa)
        return self

    def level_kappa(self, l: int, di: int = 0) -> torch.Tensor:
        """interior (z, y, x) view of the coefficient on local sub-domain di of level l (VarCoefWeights only)"""
        dd = self._dds[l]
        return dd.interior(dd.curr(di, self.kappa), di)

    def set_guess(self, fn=None):
        """u0 = fn(gz, gy, gx); default 0"""
        if fn is None:
            self._zero(0, self.u)
            self.synchronize()
        else:
            self._dds[0].fill_from_global(self.u, fn)
        return self

    def solution(self, di: int = 0) -> torch.Tensor:
        """interior (z, y, x) view of u on local sub-domain di of level 0"""
        return self._dds[0].interior(self._dds[0].curr(di, self.u), di)

    def synchronize(self):
        if self._dds[0].backend() == _C.Backend.Device and torch.cuda.is_available():
            torch.cuda.synchronize()

    # ---- the cycle ----
    def _halos(self, l, q=None):
        """valid halos of curr(q) (default u) at level l: the exchange (blocking; it orders itself after the null
        stream, where the kernels run), then the ghost cells beyond the walls"""
        dd = self._dds[l]
        dd.exchange()
        if self.boundary is not None:
            dd.apply_boundary(self.u if q is None else q)

    def _apply(self, l, weights):
        """next(u) = weights applied to curr(u) at level l"""
        dd = self._dds[l]
        self._halos(l)
        for di in range(dd.num_domains()):
            if self._box:
                box_apply(dd, di, self.u, weights)
            else:
                star_apply(dd, di, self.u, weights)

    def _smooth(self, l, sweeps):
        """damped Jacobi: u <- (I - c A) u + c f, c = omega / centre(A)"""
        dd = self._dds[l]
        if self._varcoef:
            # u + omega (f - A u) / diag(A) in one pass, ping-pong between u and v; an odd count ends with one copy
            src, dst = self.u, self.v
            for _ in range(sweeps):
                self._halos(l, src)
                for di in range(dd.num_domains()):
                    varcoef_relax(dd, di, src, self.kappa, self.f, self._weights[l], omega=self.omega, dst=dst,
                                  dst_curr=True)
                src, dst = dst, src
            if sweeps % 2:
                dd.copy(self.u, self.v)
            return
        for _ in range(sweeps):
            self._apply(l, self._smoother[l])
            dd.axpby(self.u, 1.0, self.u, self._c[l], self.f, x_curr=False)

    def _residual(self, l, stats=False):
        """r = f - A u at level l; with stats the FieldStats of r (collective)"""
        if self._varcoef:
            dd = self._dds[l]
            self._halos(l)
            for di in range(dd.num_domains()):
                varcoef_relax(dd, di, self.u, self.kappa, self.f, self._weights[l], dst=self.r, dst_curr=True)
            return dd.reduce(self.r) if stats else None
        self._apply(l, self._weights[l])
        return self._dds[l].axpby(self.r, 1.0, self.f, -1.0, self.u, y_curr=False, stats=stats)

    def _cycle(self, l):
        if l == self.levels - 1:
            self._smooth(l, self.coarse_sweeps)
            return
        fine, coarse = self._dds[l], self._dds[l + 1]
        self._smooth(l, self.nu[0])
        self._residual(l)
        for di in range(fine.num_domains()):
            restrict_apply(fine, coarse, di, self.r, self.f)
        self._zero(l + 1, self.u)
        self._cycle(l + 1)
        self._halos(l + 1)
        for di in range(fine.num_domains()):
            prolong_apply(coarse, fine, di, self.u, self.u, add=self.u)
        self._smooth(l, self.nu[1])

    def cycle(self):
        """one V(nu[0], nu[1]) cycle from the current u (asynchronous between its exchanges)"""
        self._cycle(0)

    @staticmethod
    def _finite(s, what):
        if s.nonfinite > 0:
            raise FloatingPointError(f"StarMG: {s.nonfinite} non-finite cells in {what}")

    def solve(self, tol: float = 1e-8, max_cycles: int = 50):
        """V-cycles from the current u until the true residual ||f - A u||2 / ||f||2 at level 0 is below `tol`, or
        `max_cycles` cycles: returns (cycles, relres). The residual takes one extra pass per cycle, whose axpby
        returns ||r||^2 from the same launch; `history` holds it per cycle. Collective: every rank gets the same bits
        and stops at the same cycle. f = 0 returns (0, 0.0) with u = 0; a non-finite cell raises FloatingPointError.
        Singular operators are the caller's responsibility (f must sum to zero; no projection is done)."""
        dd = self._dds[0]
        self.history = []
        sf = dd.reduce(self.f)
        self._finite(sf, "f")
        ff = sf.sum_sq
        if ff == 0:
            self.set_guess()  # an exact 0 whatever u held
            return 0, 0.0
        rel = None
        for k in range(max_cycles):
            self.cycle()
            s = self._residual(0, stats=True)
            self._finite(s, f"the residual after cycle {k + 1}")
            rel = math.sqrt(s.sum_sq / ff)
            self.history.append(rel)
            if rel < tol:
                break
        if rel is None:
            s = self._residual(0, stats=True)
            self._finite(s, "the residual")
            rel = math.sqrt(s.sum_sq / ff)
        return len(self.history), rel
