"""Operator algebra of the geometric multigrid solver (``models.StarMG``): the weights of the coarser levels and of
the damped-Jacobi smoother, computed in Python doubles from a ``_C.StarWeights`` or ``_C.BoxWeights``. The solver and
its oracle ``ops.mg_cycle_reference`` both build their weights here, so they hand the kernels the same doubles.
"""
from __future__ import annotations

import math

from .. import _C
from .box import box_to_lists, box_weights
from .star import star_to_lists, star_weights
from .varcoef import varcoef_to_lists, varcoef_weights


def _is_box(w) -> bool:
    return isinstance(w, _C.BoxWeights)


def _is_varcoef(w) -> bool:
    return isinstance(w, _C.VarCoefWeights)


def _refuse_varcoef(w, what):
    if _is_varcoef(w):
        raise TypeError(f"{what} needs a constant centre, which VarCoefWeights do not have: the diagonal "
                        f"shift - sum of h * (kappa(c) + kappa(n)) differs per cell (ops.varcoef_relax divides by it)")


def weights_center(w) -> float:
    _refuse_varcoef(w, "weights_center")
    return w.get(0, 0, 0) if _is_box(w) else w.center


def weights_sum(w) -> float:
    """the sum of all weights (math.fsum): the zeroth-order term s of A = s I + D"""
    if _is_box(w):
        return math.fsum(v for plane in box_to_lists(w) for row in plane for v in row)
    _, center, x, y, z = star_to_lists(w)
    return math.fsum([center, *x, *y, *z])


def _map(w, center_fn, off_fn):
    """a copy of w with centre center_fn(centre) and every other weight off_fn(weight)"""
    if _is_box(w):
        out = [[[off_fn(v) for v in row] for row in plane] for plane in box_to_lists(w)]
        out[1][1][1] = center_fn(w.get(0, 0, 0))
        return box_weights(out)
    r, center, x, y, z = star_to_lists(w)
    return star_weights(r, center_fn(center), *([off_fn(v) for v in ax] for ax in (x, y, z)))


def coarsened_weights(w, level: int):
    """s I + D / 4^level for A = s I + D, s = weights_sum(A): the re-discretization of A at spacing 2^level h when D
    is a second-order differential operator scaled by 1 / h^2 (Laplacian, Helmholtz, implicit diffusion). VarCoefWeights keep their shift and take h / 4^level."""
    if level == 0:
        return w
    if _is_varcoef(w):
        # shift is the zeroth-order term itself; the face scales are 1 / (2 h^2)
        shift, h = varcoef_to_lists(w)
        return varcoef_weights(shift, *(v / 4.0 ** level for v in h))
    s, q = weights_sum(w), 4.0 ** level
    return _map(w, lambda c: s + (c - s) / q, lambda v: v / q)


def smoother_weights(w, c: float):
    """I - c A: one damped-Jacobi sweep is u <- (I - c A) u + c f with c = omega / centre(A)"""
    _refuse_varcoef(w, "smoother_weights")
    return _map(w, lambda v: 1.0 - c * v, lambda v: -(c * v))


__all__ = ["weights_center", "weights_sum", "coarsened_weights", "smoother_weights"]
