"""Builders of weighted star stencils (``_C.StarWeights``) for ``star_apply`` / ``StarStencil3D``.

A star of radius R has a centre weight and, per axis x, y, z, 2R independent weights for the offsets -R..-1, +1..+R.
"""
from __future__ import annotations

from .. import _C

# central second-derivative coefficients per order: (centre, [k = 1, 2, ...])
_LAPLACIAN = {
    2: (-2.0, [1.0]),
    4: (-5.0 / 2.0, [4.0 / 3.0, -1.0 / 12.0]),
    6: (-49.0 / 18.0, [3.0 / 2.0, -3.0 / 20.0, 1.0 / 90.0]),
}


def star_weights(radius: int, center: float, x, y, z) -> _C.StarWeights:
    """Star of `radius` (1, 2 or 3) with centre weight `center`; each of x, y, z is a sequence of 2 * radius weights
    for the offsets -radius..-1, +1..+radius along that axis."""
    if radius not in (1, 2, 3):
        raise ValueError(f"star radius must be 1, 2 or 3, not {radius!r}")
    w = _C.StarWeights()
    w.radius = int(radius)
    w.center = float(center)
    for ax, (name, vals) in enumerate((("x", x), ("y", y), ("z", z))):
        vals = [float(v) for v in vals]
        if len(vals) != 2 * radius:
            raise ValueError(f"{name} needs {2 * radius} weights (offsets -{radius}..-1, +1..+{radius}), got {len(vals)}")
        for k in range(1, radius + 1):
            w.set(ax, 0, k, vals[radius - k])
            w.set(ax, 1, k, vals[radius + k - 1])
    return w


def star_to_lists(w: _C.StarWeights):
    """(radius, center, x, y, z) of a StarWeights, the axes as star_weights takes them."""
    r = w.radius
    axes = [[w.get(ax, 0, k) for k in range(r, 0, -1)] + [w.get(ax, 1, k) for k in range(1, r + 1)] for ax in range(3)]
    return r, w.center, axes[0], axes[1], axes[2]


def laplacian_star(order: int, spacing=(1, 1, 1)) -> _C.StarWeights:
    """Central-difference Laplacian of accuracy `order` (2, 4 or 6; radius order / 2) on a grid of `spacing`
    (hx, hy, hz): the standard second-derivative coefficients divided by h^2 per axis, the three centre terms summed
    in double."""
    if order not in _LAPLACIAN:
        raise ValueError(f"laplacian order must be 2, 4 or 6, not {order!r}")
    c0, side = _LAPLACIAN[order]
    if len(spacing) != 3 or any(float(h) <= 0 for h in spacing):
        raise ValueError(f"spacing must be three positive numbers, got {spacing!r}")
    center = 0.0
    axes = []
    for h in spacing:
        h2 = float(h) * float(h)
        center += c0 / h2
        axes.append([c / h2 for c in reversed(side)] + [c / h2 for c in side])
    return star_weights(order // 2, center, *axes)


def diffusion_star(order: int, alpha: float, spacing=(1, 1, 1)) -> _C.StarWeights:
    """One explicit diffusion step: identity + alpha * laplacian_star(order, spacing)."""
    r, center, x, y, z = star_to_lists(laplacian_star(order, spacing))
    a = float(alpha)
    return star_weights(r, 1.0 + a * center, [a * v for v in x], [a * v for v in y], [a * v for v in z])


__all__ = ["star_weights", "star_to_lists", "laplacian_star", "diffusion_star"]
