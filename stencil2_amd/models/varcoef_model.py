"""A variable-coefficient diffusion stencil stepped over a distributed grid, periodic or with physical boundary
conditions.

``VarCoefStencil3D`` holds two quantities, the field ``u`` and the cell coefficient ``kappa``. Each ``step()``
exchanges the face halos of both to depth 1, fills the ghost cells beyond the non-periodic faces (``boundary`` for u,
``kappa_boundary`` for kappa; None = Mirror on every non-periodic face of ``boundary``), applies ``ops.varcoef_apply``
to every local sub-domain and swaps the buffers. Results are bitwise equal to ``ops.varcoef_step_reference`` on the
gathered global grids.
"""
from __future__ import annotations

import torch

from .. import _C
from ..ops.kernels import varcoef_apply, varcoef_supported
from ..parallel.domain import DistributedDomain

_AXES = ((0, (-1, 0, 0), (1, 0, 0)), (1, (0, -1, 0), (0, 1, 0)), (2, (0, 0, -1), (0, 0, 1)))


def refuse_open(bc, what):
    """an Open face leaves its ghost cells undefined, and the operator reads them"""
    if bc is None:
        return
    for ax, lo, hi in _AXES:
        for d in (lo, hi):
            if bc.face(*d).kind == _C.FaceKind.Open:
                raise ValueError(f"{what} cannot take an Open face (axis {ax}): nothing defines the operator there")


def kappa_conditions(boundary, kappa_boundary=None):
    """the conditions of the coefficient: `kappa_boundary`, or Mirror on every non-periodic face of `boundary` (the
    coefficient of the wall cell continues beyond the wall); None for a periodic grid"""
    if kappa_boundary is not None or boundary is None:
        return kappa_boundary
    bc = _C.BoundaryConditions()
    for ax, lo, hi in _AXES:
        faces = [_C.FaceCondition.periodic() if boundary.face(*d).kind == _C.FaceKind.Periodic
                 else _C.FaceCondition.mirror() for d in (lo, hi)]
        bc.set_axis(ax, faces[0], faces[1])
    return bc


class VarCoefStencil3D:
    def __init__(self, size, w, fp64: bool = False, gpus=None, backend=None, methods=_C.MethodFlags.All, group=None,
                 axis_cost=None, tune=None, boundary=None, kappa_boundary=None):
        if not isinstance(w, _C.VarCoefWeights):
            raise ValueError(f"VarCoefStencil3D takes VarCoefWeights (ops.varcoef_weights), not {type(w).__name__}")
        if boundary is None and kappa_boundary is not None:
            raise ValueError("kappa_boundary needs boundary: the periodic faces of u and kappa are the grid's")
        refuse_open(boundary, "VarCoefStencil3D")
        refuse_open(kappa_boundary, "VarCoefStencil3D (kappa)")
        self.weights = w
        self.tune = tune
        self.dtype = torch.float64 if fp64 else torch.float32
        dd = DistributedDomain(*size, group=group)
        dd.set_radius(_C.Radius.face_edge_corner(1, 0, 0))  # face neighbours only, of u and of kappa
        dd.set_methods(methods)
        if gpus is not None:
            dd.set_gpus(list(gpus))
        if backend is not None:
            dd.set_backend(backend)
        if axis_cost is not None:  # NodeAware cut costs per axis (the cheapest axis is cut first)
            dd.set_axis_cost(_C.Dim3(*axis_cost))
        self.u = dd.add_data("u", self.dtype)
        self.kappa = dd.add_data("kappa", self.dtype)
        self.boundary = boundary
        self.kappa_boundary = kappa_conditions(boundary, kappa_boundary)
        if boundary is not None:
            dd.set_boundary_conditions(boundary)
            dd.set_boundary_conditions(self.kappa, self.kappa_boundary)
        dd.realize()
        for di in range(dd.num_domains()):
            assert varcoef_supported(dd, di, self.u, self.kappa)
        self._dd = dd
        self._size = tuple(int(v) for v in size)

    def set_kappa(self, fn):
        """kappa = fn(gz, gy, gx) (torch index tensors of global coordinates) in the interior of both of its buffers:
        swap() swaps every quantity and the kernel reads curr, so after an odd number of steps the other buffer is the
        coefficient."""
        for _ in range(2):
            self._dd.fill_from_global(self.kappa, fn)
            self._dd.swap()
        return self

    def init(self, fn=None):
        """Fill u's interior with fn(gz, gy, gx) (torch index tensors of global coordinates; default 0)."""
        if fn is None:
            def fn(gz, gy, gx):
                return torch.zeros((), dtype=self.dtype, device=gz.device) * (gz + gy + gx)
        self._dd.fill_from_global(self.u, fn)
        return self

    def step(self):
        dd = self._dd
        dd.exchange()  # blocking; orders itself after the null stream, where the kernels below run
        if self.boundary is not None:
            dd.apply_boundary()  # u and kappa: one launch per sub-domain that touches a non-periodic face
        for di in range(dd.num_domains()):
            varcoef_apply(dd, di, self.u, self.kappa, self.weights, tune=self.tune)
        dd.swap()

    def run(self, iters: int):
        for _ in range(int(iters)):
            self.step()

    def run_until(self, tol: float, max_iters: int, check_every: int = 10, norm="inf"):
        """Step until the change one step makes to u falls below `tol`: returns (iters_done, value), as
        StarStencil3D.run_until (models/until.py)."""
        from .until import run_until
        return run_until(self, self._dd.residual, [self.u], tol, max_iters, check_every, norm)

    def synchronize(self):
        if self._dd.backend() == _C.Backend.Device and torch.cuda.is_available():
            torch.cuda.synchronize()

    @property
    def domain(self):
        return self._dd

    def cells(self) -> int:
        return self._size[0] * self._size[1] * self._size[2]

    def field(self, di: int = 0, q: int = 0, curr: bool = True) -> torch.Tensor:
        """Full (z, y, x) view including halo of quantity q (0: u, 1: kappa)."""
        return self._dd.curr(di, q) if curr else self._dd.next(di, q)

    def interior(self, di: int = 0) -> torch.Tensor:
        return self._dd.interior(self.field(di, self.u), di)

    def kappa_interior(self, di: int = 0) -> torch.Tensor:
        return self._dd.interior(self.field(di, self.kappa), di)
