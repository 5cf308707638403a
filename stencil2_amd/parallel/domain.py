"""Python face of the native DistributedDomain, with zero-copy torch views of every quantity.

Parity: reference include/stencil/stencil.hpp (DistributedDomain API). The views are DLPack exports of the
runtime's halo-padded allocations: ``curr(di, q)`` has shape (z, y, x) = raw_size (interior + halo) and the padded
x pitch as its stride, so writes through the tensor are seen by the HIP kernels and vice versa.
"""
from __future__ import annotations

import torch

from .. import _C
from .process_group import get_group

_TORCH_TO_DT = {
    torch.float32: _C.DType.F32,
    torch.float64: _C.DType.F64,
    torch.int32: _C.DType.I32,
    torch.int64: _C.DType.I64,
    torch.uint8: _C.DType.U8,
    torch.int8: _C.DType.I8,
    torch.float16: _C.DType.F16,
    torch.bfloat16: _C.DType.BF16,
}


class DistributedDomain:
    """A global grid split into sub-domains (one per GPU, several per process allowed). Periodic by default;
    ``set_boundary_conditions(bc)`` / ``set_boundary_conditions(q, bc)`` (before ``realize()``) choose per face and per
    quantity how the ghost cells beyond a non-periodic face are filled (``_C.BoundaryConditions``), and
    ``apply_boundary(q=None, curr=True, stream=0)`` fills them after an exchange has landed."""

    def __init__(self, x: int, y: int, z: int, group=None):
        self._group = group if group is not None else get_group()
        self._dd = _C.DistributedDomain(int(x), int(y), int(z), self._group)
        self._dtypes: list[torch.dtype] = []

    # -------- configuration --------
    def set_radius(self, r):
        self._dd.set_radius(r)

    def add_data(self, name: str = "", dtype: torch.dtype = torch.float32) -> int:
        """Register a quantity; returns its index (the reference's DataHandle)."""
        self._dtypes.append(dtype)
        es = torch.empty((), dtype=dtype).element_size()
        return self._dd.add_data(es, name, _TORCH_TO_DT.get(dtype, _C.DType.Bytes))

    def __getattr__(self, name):
        return getattr(self._dd, name)

    @property
    def native(self):
        return self._dd

    # -------- views --------
    def domains(self):
        return [self._dd.domain(i) for i in range(self._dd.num_domains())]

    def curr(self, di: int, q: int = 0) -> torch.Tensor:
        """(z, y, x) view of the whole allocation (halo included) of the current buffer."""
        return torch.from_dlpack(self._dd.dlpack(di, q, True))

    def next(self, di: int, q: int = 0) -> torch.Tensor:
        return torch.from_dlpack(self._dd.dlpack(di, q, False))

    def interior(self, t: torch.Tensor, di: int) -> torch.Tensor:
        """Slice the interior (compute region) out of a full view."""
        d = self._dd.domain(di)
        r = d.radius()
        sz = d.size()
        return t[r.z(-1): r.z(-1) + sz.z, r.y(-1): r.y(-1) + sz.y, r.x(-1): r.x(-1) + sz.x]

    def curr_interior(self, di: int, q: int = 0) -> torch.Tensor:
        return self.interior(self.curr(di, q), di)

    def origin(self, di: int):
        return self._dd.get_origin(di)

    # -------- field reductions --------
    def reduce(self, q: int, other=None, curr: bool = True, other_curr: bool = False, local: bool = False):
        """FieldStats of quantity q over the whole grid's compute region: count, nonfinite, sum, sum_abs, sum_sq, min,
        max (and l1, l2, linf); with `other` of e = q - other, plus dot = sum of q * other. `curr` / `other_curr` pick
        each operand's curr or next buffer. Collective unless `local`; every rank returns identical bits, and the
        same call returns the same bits every time (no atomics, fixed combine order)."""
        return self._dd.reduce(int(q), None if other is None else int(other), bool(curr), bool(other_curr), bool(local))

    def norm(self, q: int, p=2, curr: bool = True) -> float:
        """the 1-, 2- or "inf"-norm of quantity q (linf is nan when a cell is not finite)"""
        if p not in (1, 2, "inf"):
            raise ValueError(f"norm p must be 1, 2 or 'inf', not {p!r}")
        s = self.reduce(q, curr=curr)
        return s.l1 if p == 1 else s.l2 if p == 2 else s.linf

    def dot(self, qa: int, qb: int) -> float:
        """sum over the grid of curr(qa) * curr(qb), accumulated in double"""
        return self.reduce(qa, other=qb, other_curr=True).dot

    def residual(self, q: int):
        """FieldStats of curr(q) - next(q): after a single step and swap, the change that step made"""
        return self.reduce(q, other=q, other_curr=False)

    # -------- field algebra --------
    def axpby(self, dst: int, a: float, x: int, b: float = 0.0, y=None, dst_curr: bool = True, x_curr: bool = True,
              y_curr: bool = True, stats: bool = False, local: bool = False, stream: int = 0):
        """dst = a * x (y None) or a * x + b * y over the compute region of every local sub-domain (`ops.field_axpby`);
        `*_curr` pick each operand's curr or next buffer, and dst may alias x and / or y. One launch per sub-domain on
        `stream`; asynchronous, not collective, returns None. With `stats` it waits for the stream and returns the
        FieldStats of the stored values from the same pass: collective unless `local`, identical bits on every rank.
        Only the compute region is written, so the halos of dst are stale: exchange before the next stencil."""
        return self._dd.axpby(int(dst), bool(dst_curr), float(a), int(x), bool(x_curr), float(b),
                              -1 if y is None else int(y), bool(y_curr), bool(stats), bool(local), stream)

    def copy(self, dst: int, src: int, dst_curr: bool = True, src_curr: bool = True):
        """dst = src over the compute regions (an exact copy: axpby with a = 1)"""
        self.axpby(dst, 1.0, src, dst_curr=dst_curr, x_curr=src_curr)

    def scale(self, q: int, a: float, curr: bool = True):
        """q = a * q over the compute regions, in place"""
        self.axpby(q, a, q, dst_curr=curr, x_curr=curr)

    def convert_from(self, src_dd, dst_q: int, src_q: int, scale: float = 1.0, dst_curr: bool = True,
                     src_curr: bool = True, stats: bool = False, local: bool = False, stream: int = 0):
        """dst_q = T_dst(scale * double(src_q)) over the compute region of every local sub-domain, src_q a quantity of
        `src_dd`: another domain with the same local partition (or this one), fp32 or fp64 on each side
        (`ops.field_convert`). Asynchronous and not collective, returns None; with `stats` it waits for the stream and
        returns the FieldStats of the stored values: collective unless `local`, identical bits on every rank. Only the
        compute region is written, so the halos of dst_q are stale: exchange before the next stencil."""
        return self._dd.convert_from(getattr(src_dd, "native", src_dd), int(dst_q), bool(dst_curr), int(src_q),
                                     bool(src_curr), float(scale), bool(stats), bool(local), stream)

    def fill_from_global(self, q: int, fn, include_halo: bool = False):
        """Set every local cell of quantity q to fn(gz, gy, gx) (torch index tensors of global coordinates)."""
        for di, d in enumerate(self.domains()):
            t = self.curr(di, q)
            org = d.accessor_origin()
            raw = d.raw_size()
            dev = t.device
            gz = torch.arange(raw.z, device=dev).view(-1, 1, 1) + org.z
            gy = torch.arange(raw.y, device=dev).view(1, -1, 1) + org.y
            gx = torch.arange(raw.x, device=dev).view(1, 1, -1) + org.x
            vals = fn(gz, gy, gx).to(t.dtype)
            if include_halo:
                t.copy_(vals.expand_as(t))
            else:
                self.interior(t, di).copy_(self.interior(vals.expand(raw.z, raw.y, raw.x), di))
        if torch.cuda.is_available():
            torch.cuda.synchronize()
