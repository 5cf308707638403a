"""Builders of variable-coefficient stencil weights (``_C.VarCoefWeights``) for ``varcoef_apply`` / ``VarCoefStencil3D``.

The operator is shift * u + sum over the six faces of h[axis] * (kappa(c) + kappa(n)) * (u(n) - u(c)): the face
coefficient is the arithmetic mean of the two cells with the 1/2 inside h, so div(kappa grad u) at spacing hx takes
h[0] = 1 / (2 hx^2). Harmonic means and separate face-coefficient fields are not provided.
"""
from __future__ import annotations

from .. import _C


def _spacing3(spacing):
    try:
        h = [float(v) for v in spacing]
    except TypeError:
        h = [float(spacing)] * 3
    if len(h) != 3 or not all(v > 0 for v in h):
        raise ValueError(f"spacing must be one positive value or three (x, y, z), got {spacing!r}")
    return h


def varcoef_weights(shift, hx, hy, hz) -> _C.VarCoefWeights:
    """Weights from the centre shift and the scales of the x, y and z faces."""
    w = _C.VarCoefWeights()
    w.shift = float(shift)
    w.h = [float(hx), float(hy), float(hz)]
    return w


def varcoef_to_lists(w: _C.VarCoefWeights):
    """(shift, [hx, hy, hz]) of a VarCoefWeights; varcoef_weights(shift, *h) rebuilds it."""
    return w.shift, list(w.h)


def diffusion_varcoef(alpha: float, spacing=(1, 1, 1)) -> _C.VarCoefWeights:
    """One explicit diffusion step u + alpha div(kappa grad u): shift = 1, h[a] = alpha / (2 h_a^2)."""
    a = float(alpha)
    return varcoef_weights(1.0, *(a / (2.0 * (h * h)) for h in _spacing3(spacing)))


def operator_varcoef(sigma: float, spacing=(1, 1, 1)) -> _C.VarCoefWeights:
    """The operator sigma - div(kappa grad): shift = sigma, h[a] = -1 / (2 h_a^2). Symmetric, and positive definite
    for kappa > 0 and sigma > 0 (sigma = 0 with periodic or all-Mirror walls is singular)."""
    return varcoef_weights(float(sigma), *(-1.0 / (2.0 * (h * h)) for h in _spacing3(spacing)))


__all__ = ["varcoef_weights", "varcoef_to_lists", "diffusion_varcoef", "operator_varcoef"]
