"""A weighted star stencil (radius 1-3, caller-supplied weights) stepped over a distributed grid, periodic or with
physical boundary conditions.

``StarStencil3D`` is a thin Python class over ``parallel.DistributedDomain``: each ``step()`` exchanges the face halos
to depth ``weights.radius``, fills the ghost cells beyond the non-periodic faces (``boundary``: a
``BoundaryConditions``; None = periodic), applies ``ops.star_apply`` to every quantity of every local sub-domain and
swaps the buffers. Results are bitwise equal to ``ops.star_step_reference`` on the gathered global grid.
"""
from __future__ import annotations

import torch

from .. import _C
from ..ops.kernels import star_apply, star_supported
from ..parallel.domain import DistributedDomain


class StarStencil3D:
    def __init__(self, size, weights, quantities: int = 1, fp64: bool = False, gpus=None, backend=None,
                 methods=_C.MethodFlags.All, group=None, axis_cost=None, tune=None, boundary=None):
        if weights.radius not in (1, 2, 3):
            raise ValueError(f"star radius must be 1, 2 or 3, not {weights.radius}")
        self.weights = weights
        self.tune = tune
        self.dtype = torch.float64 if fp64 else torch.float32
        dd = DistributedDomain(*size, group=group)
        dd.set_radius(_C.Radius.face_edge_corner(weights.radius, 0, 0))  # a star reads faces only
        dd.set_methods(methods)
        if gpus is not None:
            dd.set_gpus(list(gpus))
        if backend is not None:
            dd.set_backend(backend)
        if axis_cost is not None:  # NodeAware cut costs per axis (the cheapest axis is cut first)
            dd.set_axis_cost(_C.Dim3(*axis_cost))
        self._qs = [dd.add_data(f"u{q}", self.dtype) for q in range(quantities)]
        self.boundary = boundary
        if boundary is not None:
            dd.set_boundary_conditions(boundary)
        dd.realize()
        for di in range(dd.num_domains()):
            for q in self._qs:
                assert star_supported(dd, di, q, weights)
        self._dd = dd
        self._size = tuple(int(v) for v in size)

    def init(self, fn=None):
        """Fill every quantity's interior with fn(gz, gy, gx) (torch index tensors of global coordinates; default 0)."""
        if fn is None:
            def fn(gz, gy, gx):
                return torch.zeros((), dtype=self.dtype, device=gz.device) * (gz + gy + gx)
        for q in self._qs:
            self._dd.fill_from_global(q, fn)
        return self

    def step(self):
        dd = self._dd
        dd.exchange()  # blocking; orders itself after the null stream, where the kernels below run
        if self.boundary is not None:
            dd.apply_boundary()  # one launch per sub-domain that touches a non-periodic face
        for di in range(dd.num_domains()):
            for q in self._qs:
                star_apply(dd, di, q, self.weights, tune=self.tune)
        dd.swap()

    def run(self, iters: int):
        for _ in range(int(iters)):
            self.step()

    def run_until(self, tol: float, max_iters: int, check_every: int = 10, norm="inf"):
        """Step until the change made by one step falls below `tol`: returns (iters_done, value). Advances in blocks of
        `check_every` steps (run(check_every - 1), then one step()), synchronizes and evaluates the `norm` (1, 2 or
        "inf"; over every quantity) of curr - next over the compute regions, the change made by the block's last step;
        stops at the first check with value < tol, or at `max_iters`. Raises FloatingPointError as soon as a check
        sees a non-finite cell. Collective: every rank computes the same value. Holds for every configuration of
        this model (models/until.py). The default check_every = 10 is a bytes estimate, not a measurement: the
        two-operand reduction reads about as many bytes as one single step moves, so a check every tenth step costs on
        the order of a tenth of the steps ("Field reductions", has the measured ratio)."""
        from .until import run_until
        return run_until(self, self._dd.residual, self._qs, tol, max_iters, check_every, norm)

    def synchronize(self):
        if self._dd.backend() == _C.Backend.Device and torch.cuda.is_available():
            torch.cuda.synchronize()

    @property
    def domain(self):
        return self._dd

    def cells(self) -> int:
        return self._size[0] * self._size[1] * self._size[2]

    def field(self, di: int = 0, q: int = 0, curr: bool = True) -> torch.Tensor:
        """Full (z, y, x) view including halo."""
        return self._dd.curr(di, q) if curr else self._dd.next(di, q)

    def interior(self, di: int = 0, q: int = 0) -> torch.Tensor:
        return self._dd.interior(self.field(di, q), di)
