"""Builders of weighted 27-point box stencils (``_C.BoxWeights``) for ``box_apply`` / ``BoxStencil3D``.

A box has 27 independent weights w[dz][dy][dx], one per neighbour offset (dx, dy, dz) with every component in
-1, 0, +1. Nested lists are indexed [dz + 1][dy + 1][dx + 1], the order in which ``box_apply`` sums the terms.
"""
from __future__ import annotations

from .. import _C

_OFFS = (-1, 0, 1)

# compact Laplacians: coefficient per |d|_1 class (centre, face, edge, corner) and the common divisor
_LAPLACIAN_BOX = {
    7: ((-6.0, 1.0, 0.0, 0.0), 1.0),
    19: ((-24.0, 2.0, 1.0, 0.0), 6.0),
    27: ((-128.0, 14.0, 3.0, 1.0), 30.0),
}


def box_weights(w) -> _C.BoxWeights:
    """Box from a nested 3 x 3 x 3 sequence w[dz + 1][dy + 1][dx + 1]."""
    try:
        planes = [[[float(v) for v in row] for row in plane] for plane in w]
    except TypeError:
        raise ValueError("box weights must be a nested 3 x 3 x 3 sequence [dz][dy][dx]") from None
    if len(planes) != 3 or any(len(p) != 3 for p in planes) or any(len(r) != 3 for p in planes for r in p):
        raise ValueError("box weights must be a nested 3 x 3 x 3 sequence [dz][dy][dx]")
    b = _C.BoxWeights()
    for dz in _OFFS:
        for dy in _OFFS:
            for dx in _OFFS:
                b.set(dz, dy, dx, planes[dz + 1][dy + 1][dx + 1])
    return b


def box_to_lists(w: _C.BoxWeights):
    """The nested 3 x 3 x 3 list [dz + 1][dy + 1][dx + 1] of a BoxWeights, as box_weights takes it."""
    return [[[w.get(dz, dy, dx) for dx in _OFFS] for dy in _OFFS] for dz in _OFFS]


def _by_class(coeffs):
    """box whose weight depends on the number of non-zero offset components only (centre, face, edge, corner)"""
    return box_weights([[[coeffs[abs(dz) + abs(dy) + abs(dx)] for dx in _OFFS] for dy in _OFFS] for dz in _OFFS])


def box_from_star(star: _C.StarWeights) -> _C.BoxWeights:
    """The radius-1 star as a box: centre and six face weights, edges and corners 0."""
    if star.radius != 1:
        raise ValueError(f"only a radius-1 star fits a box, not radius {star.radius}")
    b = _C.BoxWeights()
    b.set(0, 0, 0, star.center)
    for ax in range(3):
        for side, s in ((0, -1), (1, 1)):
            d = [0, 0, 0]  # (dz, dy, dx)
            d[2 - ax] = s
            b.set(d[0], d[1], d[2], star.get(ax, side, 1))
    return b


def laplacian_box(points: int, spacing: float = 1.0) -> _C.BoxWeights:
    """Compact Laplacian on 7, 19 or 27 points with one grid spacing h for all axes; per class (centre, face, edge,
    corner): 7 -> (-6, 1, 0, 0), 19 -> (-24, 2, 1, 0) / 6, 27 -> (-128, 14, 3, 1) / 30, each divided by h^2. Both
    compact sets sum to zero and have second moment 2 per axis."""
    if points not in _LAPLACIAN_BOX:
        raise ValueError(f"laplacian_box points must be 7, 19 or 27, not {points!r}")
    h = float(spacing)
    if not h > 0:
        raise ValueError(f"spacing must be positive, got {spacing!r}")
    coeffs, div = _LAPLACIAN_BOX[points]
    den = div * (h * h)
    return _by_class([c / den for c in coeffs])


def diffusion_box(points: int, alpha: float, spacing: float = 1.0) -> _C.BoxWeights:
    """One explicit diffusion step: identity + alpha * laplacian_box(points, spacing)."""
    w = box_to_lists(laplacian_box(points, spacing))
    a = float(alpha)
    out = [[[a * v for v in row] for row in plane] for plane in w]
    out[1][1][1] = 1.0 + out[1][1][1]
    return box_weights(out)


def smoothing_box() -> _C.BoxWeights:
    """Binomial smoothing: the tensor product of [1, 2, 1] / 4, i.e. 2^(number of zero offset components) / 64. All
    weights are exact in binary and sum to 1 exactly."""
    return _by_class([8.0 / 64.0, 4.0 / 64.0, 2.0 / 64.0, 1.0 / 64.0])


__all__ = ["box_weights", "box_to_lists", "box_from_star", "laplacian_box", "diffusion_box", "smoothing_box"]
