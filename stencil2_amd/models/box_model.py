"""A weighted 27-point box stencil (caller-supplied weights) stepped over a distributed grid, periodic or with
physical boundary conditions.

``BoxStencil3D`` is ``StarStencil3D``'s twin for ``ops.box_apply``: each ``step()`` exchanges the face, edge and corner
halos to depth 1 (all 26 directions), fills the ghost cells beyond the non-periodic faces (``boundary``: a
``BoundaryConditions``; None = periodic; edge and corner ghost cells compose x, then y, then z), applies
``ops.box_apply`` to every quantity of every local sub-domain and swaps the buffers. Results are bitwise equal to
``ops.box_step_reference`` on the gathered global grid.
"""
from __future__ import annotations

import torch

from .. import _C
from ..ops.kernels import box_apply, box_supported
from ..parallel.domain import DistributedDomain


class BoxStencil3D:
    def __init__(self, size, weights, quantities: int = 1, fp64: bool = False, gpus=None, backend=None,
                 methods=_C.MethodFlags.All, group=None, axis_cost=None, tune=None, boundary=None):
        if not isinstance(weights, _C.BoxWeights):
            raise ValueError(f"BoxStencil3D takes BoxWeights (ops.box_weights), not {type(weights).__name__}")
        self.weights = weights
        self.tune = tune
        self.dtype = torch.float64 if fp64 else torch.float32
        dd = DistributedDomain(*size, group=group)
        dd.set_radius(_C.Radius.face_edge_corner(1, 1, 1))  # a box reads faces, edges and corners
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
                assert box_supported(dd, di, q)
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
                box_apply(dd, di, q, self.weights, tune=self.tune)
        dd.swap()

    def run(self, iters: int):
        for _ in range(int(iters)):
            self.step()

    def run_until(self, tol: float, max_iters: int, check_every: int = 10, norm="inf"):
        """Step until the change made by one step falls below `tol`: returns (iters_done, value), as
        StarStencil3D.run_until (models/until.py)."""
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
