"""Pure-torch references of the runtime's semantics (periodic halos, Jacobi3D, Astaroth proxy).

The operation order matches the reference CUDA kernels (bin/jacobi3d.cu:72-83: +x,-x,+y,-y,+z,-z then /6;
bin/astaroth_sim.cu:72-81: -x,-y,-z,+x,+y,+z then /6), so fp32 results are expected to be bitwise equal to the HIP
kernels. Sphere membership uses the exact integer form of the reference's truncated float sqrt:
floor(sqrt(d2)) <= R  <=>  d2 < (R+1)^2.
"""
from __future__ import annotations

import math

import torch


def periodic_gather(g: torch.Tensor, origin, raw_size) -> torch.Tensor:
    """Values of the (z, y, x) global periodic grid `g` on the box starting at global `origin` (x, y, z)."""
    Z, Y, X = g.shape
    ox, oy, oz = origin
    rx, ry, rz = raw_size
    iz = (torch.arange(rz) + oz) % Z
    iy = (torch.arange(ry) + oy) % Y
    ix = (torch.arange(rx) + ox) % X
    return g[iz][:, iy][:, :, ix]


def jacobi_spheres(size):
    """(hot_xyz, cold_xyz, radius) for a global grid of `size` (x, y, z) (bin/jacobi3d.cu:45-50)."""
    X, Y, Z = size
    hot = (X // 3, Y // 2, Z // 2)
    cold = (X * 2 // 3, Y // 2, Z // 2)
    return hot, cold, X // 10


def _sphere_masks(shape_zyx, size_xyz, device):
    Z, Y, X = shape_zyx
    hot, cold, R = jacobi_spheres(size_xyz)
    z = torch.arange(Z, device=device).view(-1, 1, 1)
    y = torch.arange(Y, device=device).view(1, -1, 1)
    x = torch.arange(X, device=device).view(1, 1, -1)
    r1 = (R + 1) ** 2
    dh = (x - hot[0]) ** 2 + (y - hot[1]) ** 2 + (z - hot[2]) ** 2
    dc = (x - cold[0]) ** 2 + (y - cold[1]) ** 2 + (z - cold[2]) ** 2
    return dh < r1, dc < r1


def _div6(val: torch.Tensor) -> torch.Tensor:
    """IEEE val / 6 on any device. PyTorch's GPU kernel turns a division by a Python / CPU scalar into a
    multiplication by its (rounded) reciprocal, which differs in the last bit; a divisor tensor on the same device
    keeps the true division the kernels implement."""
    if val.device.type == "cpu":
        return val / 6
    return val / torch.full((), 6, dtype=val.dtype, device=val.device)


def jacobi_step_reference(u: torch.Tensor) -> torch.Tensor:
    """One Jacobi3D iteration on a periodic global (z, y, x) grid."""
    Z, Y, X = u.shape
    px = torch.roll(u, -1, 2)
    mx = torch.roll(u, 1, 2)
    py = torch.roll(u, -1, 1)
    my = torch.roll(u, 1, 1)
    pz = torch.roll(u, -1, 0)
    mz = torch.roll(u, 1, 0)
    val = torch.zeros_like(u) + px  # leading 0 + as in the reference kernel (sign of zero)
    val = val + mx
    val = val + py
    val = val + my
    val = val + pz
    val = val + mz
    val = _div6(val)
    hot, cold = _sphere_masks(u.shape, (X, Y, Z), u.device)
    val = torch.where(hot, torch.ones_like(val), val)
    val = torch.where(cold & ~hot, torch.zeros_like(val), val)
    return val


def astaroth_step_reference(u: torch.Tensor) -> torch.Tensor:
    """One Astaroth-proxy iteration (6-neighbour mean) on a periodic global (z, y, x) grid."""
    mx = torch.roll(u, 1, 2)
    my = torch.roll(u, 1, 1)
    mz = torch.roll(u, 1, 0)
    px = torch.roll(u, -1, 2)
    py = torch.roll(u, -1, 1)
    pz = torch.roll(u, -1, 0)
    val = torch.zeros_like(u) + mx
    val = val + my
    val = val + mz
    val = val + px
    val = val + py
    val = val + pz
    return _div6(val)


def astaroth_init_reference(size_xyz, radius: int, period: float, dtype=torch.float32) -> torch.Tensor:
    """Global interior initial condition of the Astaroth proxy: sin(2*pi'/period*(g+r)) summed over axes, where
    pi' = 3.14159 and (g + r) is the raw allocation index of the owning sub-domain (bin/astaroth_sim.cu:50-53)."""
    X, Y, Z = size_xyz
    k = 2 * 3.14159 / period
    z = torch.arange(Z, dtype=torch.float64).view(-1, 1, 1) + radius
    y = torch.arange(Y, dtype=torch.float64).view(1, -1, 1) + radius
    x = torch.arange(X, dtype=torch.float64).view(1, 1, -1) + radius
    return torch.sin(k * x + k * y + k * z).to(dtype)


def star_step_reference(u: torch.Tensor, weights, boundary=None) -> torch.Tensor:
    """One weighted star step (`weights`: _C.StarWeights, see ops.star) on a global (z, y, x) grid: the oracle of
    `star_apply`. acc = center * u, then per axis x, y, z and k = 1..radius: acc + w[-k] * u(c - k), then
    acc + w[+k] * u(c + k). The weights are 0-dim tensors of u's dtype (one conversion from double) and every product
    and every sum is a separate op, so each is rounded on its own in that dtype. `boundary` (_C.BoundaryConditions):
    the neighbours beyond a non-periodic face come from `pad_reference`; None is the periodic grid."""
    def wt(v):
        return torch.tensor(v, dtype=torch.float64).to(u.dtype).to(u.device)

    R = weights.radius
    if boundary is None:
        def nb(k, dim):  # u(c - k e)
            return torch.roll(u, k, dim)
    else:
        p = pad_reference(u, R, boundary)
        Z, Y, X = u.shape

        def nb(k, dim):
            lo = [R, R, R]
            lo[dim] -= k
            return p[lo[0]:lo[0] + Z, lo[1]:lo[1] + Y, lo[2]:lo[2] + X]

    acc = wt(weights.center) * u
    for ax, dim in enumerate((2, 1, 0)):
        for k in range(1, R + 1):
            term = wt(weights.get(ax, 0, k)) * nb(k, dim)  # u(c - k e)
            acc = acc + term
            term = wt(weights.get(ax, 1, k)) * nb(-k, dim)  # u(c + k e)
            acc = acc + term
    return acc


def box_step_reference(u: torch.Tensor, weights, boundary=None) -> torch.Tensor:
    """One weighted 27-point box step (`weights`: _C.BoxWeights, see ops.box) on a global (z, y, x) grid: the oracle of
    `box_apply`. acc = w(-1, -1, -1) * u(c + (-1, -1, -1)), then for every later (dz, dy, dx) in lexicographic order,
    dz slowest and dx fastest: acc + w(dz, dy, dx) * u(c + (dx, dy, dz)). The weights are 0-dim tensors of u's dtype
    (one conversion from double) and every product and every sum is a separate op, so each is rounded on its own in
    that dtype. `boundary` (_C.BoundaryConditions): the neighbours beyond a non-periodic face, edge or corner come from
    `pad_reference` (x, then y, then z); None is the periodic grid."""
    def wt(v):
        return torch.tensor(v, dtype=torch.float64).to(u.dtype).to(u.device)

    if boundary is None:
        def nb(dz, dy, dx):  # u(c + (dx, dy, dz))
            return torch.roll(u, (-dz, -dy, -dx), (0, 1, 2))
    else:
        p = pad_reference(u, 1, boundary)
        Z, Y, X = u.shape

        def nb(dz, dy, dx):
            return p[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]

    acc = None
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                term = wt(weights.get(dz, dy, dx)) * nb(dz, dy, dx)
                acc = term if acc is None else acc + term
    return acc


def varcoef_step_reference(u: torch.Tensor, kappa: torch.Tensor, w, boundary=None, kappa_boundary=None) -> torch.Tensor:
    """One variable-coefficient step (`w`: _C.VarCoefWeights, see ops.varcoef) on global (z, y, x) grids: the oracle of
    `varcoef_apply`. acc = shift * u, then per axis x, y, z first the low face, then the high face:
    ks = kappa + kappa(n); d = u(n) - u; f = ks * d; t = h[axis] * f; acc = acc + t. shift and h are 0-dim tensors of
    u's dtype (one conversion from double) and every sum, difference and product is a separate op, so each is rounded
    on its own in that dtype. `boundary` / `kappa_boundary` (_C.BoundaryConditions): the neighbours of u / kappa beyond
    a non-periodic face come from `pad_reference`; None is the periodic grid."""
    def wt(v):
        return torch.tensor(v, dtype=torch.float64).to(u.dtype).to(u.device)

    def neighbours(g, bc):
        if bc is None:
            return lambda k, dim: torch.roll(g, k, dim)  # g(c - k e)
        p = pad_reference(g, 1, bc)
        Z, Y, X = g.shape

        def nb(k, dim):
            lo = [1, 1, 1]
            lo[dim] -= k
            return p[lo[0]:lo[0] + Z, lo[1]:lo[1] + Y, lo[2]:lo[2] + X]
        return nb

    un, kn = neighbours(u, boundary), neighbours(kappa, kappa_boundary)
    h = list(w.h)
    acc = wt(w.shift) * u
    for ax, dim in enumerate((2, 1, 0)):
        for k in (1, -1):  # c - e, then c + e
            ks = kappa + kn(k, dim)
            d = un(k, dim) - u
            f = ks * d
            t = wt(h[ax]) * f
            acc = acc + t
    return acc


def varcoef_relax_reference(u: torch.Tensor, kappa: torch.Tensor, f: torch.Tensor, w, omega=None, boundary=None,
                            kappa_boundary=None) -> torch.Tensor:
    """The residual (omega None) or one damped-Jacobi sweep of the variable-coefficient operator on global (z, y, x)
    grids: the oracle of `varcoef_relax`. acc as `varcoef_step_reference`, and beside it dg = shift, then per axis
    x, y, z first the low face, then the high face: ks = kappa + kappa(n) (the sum acc uses); g = h[axis] * ks;
    dg = dg - g. r = f - acc; the residual is r, the sweep q = r / dg; s = omega * q; u + s. shift, h and omega are
    0-dim tensors of u's dtype (one conversion from double) and every sum, difference, product and quotient is a
    separate op on tensors, so each is rounded on its own in that dtype (the quotient is a true division: the divisor
    is a tensor). `boundary` / `kappa_boundary` as in `varcoef_step_reference`."""
    def wt(v):
        return torch.tensor(v, dtype=torch.float64).to(u.dtype).to(u.device)

    def neighbours(g, bc):
        if bc is None:
            return lambda k, dim: torch.roll(g, k, dim)  # g(c - k e)
        p = pad_reference(g, 1, bc)
        Z, Y, X = g.shape

        def nb(k, dim):
            lo = [1, 1, 1]
            lo[dim] -= k
            return p[lo[0]:lo[0] + Z, lo[1]:lo[1] + Y, lo[2]:lo[2] + X]
        return nb

    un, kn = neighbours(u, boundary), neighbours(kappa, kappa_boundary)
    h = list(w.h)
    acc = wt(w.shift) * u
    dg = torch.zeros_like(u) + wt(w.shift)
    for ax, dim in enumerate((2, 1, 0)):
        for k in (1, -1):  # c - e, then c + e
            ks = kappa + kn(k, dim)
            d = un(k, dim) - u
            t = wt(h[ax]) * (ks * d)
            acc = acc + t
            g = wt(h[ax]) * ks
            dg = dg - g
    r = f - acc
    if omega is None:
        return r
    q = r / dg
    s = wt(float(omega)) * q
    return u + s


def axpby_reference(a, x: torch.Tensor, b=None, y=None) -> torch.Tensor:
    """a * x, or a * x + b * y: the oracle of `field_axpby`. a and b are 0-dim tensors of x's dtype (one conversion
    from double), and each product and the sum is a separate op, so each is rounded on its own in that dtype. A zero
    coefficient is multiplied like any other (NaN and Inf propagate)."""
    def ct(v):
        return torch.tensor(float(v), dtype=torch.float64).to(x.dtype).to(x.device)

    t = ct(a) * x
    if y is None:
        return t
    s = ct(b) * y
    return t + s


def convert_reference(x: torch.Tensor, scale=1.0, dtype=None) -> torch.Tensor:
    """dtype(scale * double(x)): the oracle of `field_convert`. One product in double, then one conversion to `dtype`
    (default x's): round to nearest even, overflow to +-inf, subnormals kept. scale = 1 is an exact cast."""
    t = torch.tensor(float(scale), dtype=torch.float64).to(x.device) * x.double()
    return t.to(x.dtype if dtype is None else dtype)


# ---- physical boundary conditions (csrc/include/stencil/core/boundary.hpp) ----
_FACES = ((0, (-1, 0, 0), (1, 0, 0)), (1, (0, -1, 0), (0, 1, 0)), (2, (0, 0, -1), (0, 0, 1)))  # axis, low dir, high dir


def _kind_name(cond):
    return str(cond.kind).split(".")[-1]


def _anti_c(value, dtype, device):
    """T(2.0 * v): the double product, converted to the field's type once"""
    return torch.tensor(2.0 * value, dtype=torch.float64).to(dtype).to(device)


def pad_reference(u_global: torch.Tensor, radius: int, bc) -> torch.Tensor:
    """The global (z, y, x) grid padded by `radius` cells on every side, sequentially along x, then y, then z, each
    pass over the whole padded extent of the axes before it: periodic axes wrapped, Constant faces T(v), Mirror faces
    the mirror cell, AntiMirror faces T(2.0 * v) - mirror cell (one subtraction in the field's type). Cells beyond an
    Open face are NaN (nothing defines them)."""
    r = int(radius)
    p = u_global
    for ax, lo_dir, hi_dir in _FACES:
        dim = 2 - ax
        n = p.shape[dim]
        conds = (bc.face(*lo_dir), bc.face(*hi_dir))
        parts = []
        for side, cond in enumerate(conds):
            k = _kind_name(cond)
            if k == "Periodic":
                idx = torch.arange(n - r, n) if side == 0 else torch.arange(0, r)
                g = p.index_select(dim, (idx % n).to(p.device))
            elif k == "Open":
                shape = list(p.shape)
                shape[dim] = r
                g = torch.full(shape, float("nan"), dtype=p.dtype, device=p.device)
            elif k == "Constant":
                shape = list(p.shape)
                shape[dim] = r
                g = torch.full(shape, 0, dtype=p.dtype, device=p.device) + \
                    torch.tensor(cond.value, dtype=torch.float64).to(p.dtype).to(p.device)
            else:
                # ghost at distance k outside <- interior at distance k inside: low face r-1..0, high face n-1..n-r
                idx = torch.arange(r - 1, -1, -1) if side == 0 else torch.arange(n - 1, n - 1 - r, -1)
                if r > n:
                    raise ValueError(f"mirror of {r} cells on an axis of {n}")
                g = p.index_select(dim, idx.to(p.device))
                if k == "AntiMirror":
                    g = _anti_c(cond.value, p.dtype, p.device) - g
            parts.append(g)
        p = torch.cat([parts[0], p, parts[1]], dim=dim)
    return p


def boundary_fill_reference(raw: torch.Tensor, origin, size, radius_lo, radius_hi, grid, bc, return_mask: bool = False):
    """The composed map of csrc/include/stencil/kernels/boundary_fill.hpp applied to one sub-domain's raw (z, y, x)
    tensor (halo included; a copy is returned): `origin` / `size` (x, y, z) of the sub-domain, `radius_lo` /
    `radius_hi` its face radii per axis (x, y, z), `grid` the global size. For every cell resolve z, then y, then x:
    beyond a Constant face the chain ends with T(v); beyond Mirror / AntiMirror the coordinate is reflected; inside,
    in an exchanged halo, or beyond an Open face after an earlier axis resolved it stays; then the source cell is
    loaded and the AntiMirror subtractions applied x, then y, then z. Cells whose first face is Open, and cells beyond
    no non-periodic face, keep their content. `return_mask`: also the boolean mask of the cells written."""
    rawz, rawy, rawx = raw.shape
    ext = (rawx, rawy, rawz)
    dev = raw.device
    coords = [None, None, None]
    coords[0] = torch.arange(rawx, device=dev).view(1, 1, -1).expand(rawz, rawy, rawx).clone()
    coords[1] = torch.arange(rawy, device=dev).view(1, -1, 1).expand(rawz, rawy, rawx).clone()
    coords[2] = torch.arange(rawz, device=dev).view(-1, 1, 1).expand(rawz, rawy, rawx).clone()
    seen = torch.zeros(raw.shape, dtype=torch.bool, device=dev)
    skip = torch.zeros_like(seen)
    is_const = torch.zeros_like(seen)
    const_v = torch.zeros_like(raw)
    anti = [None, None, None]  # per axis: (mask, c tensor)
    for ax in (2, 1, 0):
        _, lo_dir, hi_dir = _FACES[ax]
        lo, hi = 0, ext[ax]
        conds = [None, None]
        if _kind_name(bc.face(*lo_dir)) != "Periodic" and origin[ax] == 0 and radius_lo[ax] > 0:
            lo, conds[0] = radius_lo[ax], bc.face(*lo_dir)
        if _kind_name(bc.face(*hi_dir)) != "Periodic" and origin[ax] + size[ax] == grid[ax] and radius_hi[ax] > 0:
            hi, conds[1] = radius_lo[ax] + size[ax], bc.face(*hi_dir)
        amask = torch.zeros_like(seen)
        aval = torch.zeros_like(raw)
        c = coords[ax]
        for side, cond in enumerate(conds):
            if cond is None:
                continue
            beyond = ((c < lo) if side == 0 else (c >= hi)) & ~is_const & ~skip
            k = _kind_name(cond)
            if k == "Open":
                skip |= beyond & ~seen
                continue
            seen |= beyond
            if k == "Constant":
                const_v = torch.where(beyond, torch.tensor(cond.value, dtype=torch.float64).to(raw.dtype).to(dev), const_v)
                is_const |= beyond
                continue
            refl = (2 * lo - 1 - c) if side == 0 else (2 * hi - 1 - c)
            if k == "AntiMirror":
                amask |= beyond
                aval = torch.where(beyond, _anti_c(cond.value, raw.dtype, dev), aval)
            c = torch.where(beyond, refl, c)
        coords[ax] = c
        anti[ax] = (amask, aval)
    v = raw[coords[2], coords[1], coords[0]]
    v = torch.where(is_const, const_v, v)
    for ax in (0, 1, 2):
        amask, aval = anti[ax]
        v = torch.where(amask, aval - v, v)
    written = seen & ~skip
    out = torch.where(written, v, raw)
    return (out, written) if return_mask else out


# ---- grid transfer and the multigrid cycle (csrc/include/stencil/kernels/grid_transfer.hpp) ----
def restrict_reference(r: torch.Tensor) -> torch.Tensor:
    """Cell-centred full weighting of a global (z, y, x) grid with even extents: the oracle of `restrict_apply`. The 8
    fine cells under a coarse cell are summed along x, then y, then z, each sum a separate op, then scaled by 0.125."""
    sx = r[:, :, 0::2] + r[:, :, 1::2]
    sy = sx[:, 0::2] + sx[:, 1::2]
    return 0.125 * (sy[0::2] + sy[1::2])


def _interp_reference(p: torch.Tensor, ax: int) -> torch.Tensor:
    """p padded by one cell along ax: fine cell 2 I is 0.75 p(I) + 0.25 p(I - 1), fine cell 2 I + 1 is
    0.75 p(I) + 0.25 p(I + 1)"""
    n = p.shape[ax] - 2
    c, lo, hi = p.narrow(ax, 1, n), p.narrow(ax, 0, n), p.narrow(ax, 2, n)
    return torch.stack([0.75 * c + 0.25 * lo, 0.75 * c + 0.25 * hi], ax + 1).flatten(ax, ax + 1)


def prolong_reference(c: torch.Tensor, boundary=None, add=None) -> torch.Tensor:
    """Trilinear cell-centred prolongation of a global (z, y, x) coarse grid to twice the extents: the oracle of
    `prolong_apply`. The grid is padded by one cell (`pad_reference(c, 1, boundary)`; None: the periodic wrap) and
    interpolated along x, then y, then z with weights 0.75 (near) and 0.25 (far), every product and sum a separate op;
    with `add` the result is add + P c (one more sum, add on the left)."""
    if boundary is None:
        p = c
        for dim in (2, 1, 0):
            n = p.shape[dim]
            p = torch.cat([p.narrow(dim, n - 1, 1), p, p.narrow(dim, 0, 1)], dim=dim)
    else:
        p = pad_reference(c, 1, boundary)
    v = _interp_reference(_interp_reference(_interp_reference(p, 2), 1), 0)
    return v if add is None else add + v


def mg_cycle_reference(u: torch.Tensor, f: torch.Tensor, weights_per_level, bc, nu=(2, 2), omega: float = 6.0 / 7.0,
                       coarse_sweeps: int = 32) -> torch.Tensor:
    """One V-cycle of `models.StarMG` on gathered global (z, y, x) grids, with the same scalars in the same order: the
    oracle of `StarMG.cycle`. `weights_per_level[l]` is the operator of level l (StarWeights or BoxWeights), `bc` the
    conditions of u at level 0 (None: periodic); coarser levels take its homogeneous twin. A smoothing sweep is
    u <- 1.0 * (S u) + c * f with c = omega / centre(A_l) and S = `ops.smoother_weights(A_l, c)`; the residual is
    1.0 * f + (-1.0) * (A_l u); the coarse problem starts from 0 and the coarsest level runs `coarse_sweeps` sweeps.
    Returns u after the cycle. The smoother's weights and the homogeneous conditions are built by the solver's own
    helpers (`ops.smoother_weights`, `models.star_cg._conditions`): the oracle checks the cycle's composition and
    arithmetic, not those two constructions, which the convergence limits of the tests guard."""
    from .multigrid import smoother_weights, weights_center
    from .. import _C
    from ..models.star_cg import _conditions

    hom = None if bc is None else _conditions(bc, True)
    last = len(weights_per_level) - 1

    def cycle(level, u, f, cond):
        A = weights_per_level[level]
        step = box_step_reference if isinstance(A, _C.BoxWeights) else star_step_reference
        c = omega / weights_center(A)
        S = smoother_weights(A, c)

        def smooth(u, sweeps):
            for _ in range(sweeps):
                u = axpby_reference(1.0, step(u, S, boundary=cond), c, f)
            return u

        if level == last:
            return smooth(u, coarse_sweeps)
        u = smooth(u, nu[0])
        r = axpby_reference(1.0, f, -1.0, step(u, A, boundary=cond))
        e = cycle(level + 1, torch.zeros_like(restrict_reference(r)), restrict_reference(r), hom)
        u = prolong_reference(e, boundary=hom, add=u)
        return smooth(u, nu[1])

    return cycle(0, u, f, bc)


def varcoef_mg_cycle_reference(u: torch.Tensor, f: torch.Tensor, kappa: torch.Tensor, weights_per_level, bc,
                               kappa_bc=None, nu=(2, 2), omega: float = 6.0 / 7.0, coarse_sweeps: int = 32) -> torch.Tensor:
    """One V-cycle of `models.StarMG` on `VarCoefWeights`, on gathered global (z, y, x) grids with the same scalars in
    the same order: the oracle of `StarMG.cycle` for the variable-coefficient operator. `weights_per_level[l]` is the
    VarCoefWeights of level l; kappa of level l + 1 is `restrict_reference` of level l's; `bc` the conditions of u at
    level 0 (None: periodic), coarser levels take its homogeneous twin; every level's kappa is padded with `kappa_bc`
    (None with walls: Mirror on every non-periodic face of `bc`). A smoothing sweep is `varcoef_relax_reference` with
    `omega`, the residual the same with omega None; the coarse problem starts from 0 and the coarsest level runs
    `coarse_sweeps` sweeps. Returns u after the cycle."""
    from ..models.star_cg import _conditions
    from ..models.varcoef_model import kappa_conditions

    hom = None if bc is None else _conditions(bc, True)
    kbc = None if bc is None else kappa_conditions(bc, kappa_bc)
    last = len(weights_per_level) - 1

    def cycle(level, u, f, kappa, cond):
        A = weights_per_level[level]

        def smooth(u, sweeps):
            for _ in range(sweeps):
                u = varcoef_relax_reference(u, kappa, f, A, omega=omega, boundary=cond, kappa_boundary=kbc)
            return u

        if level == last:
            return smooth(u, coarse_sweeps)
        u = smooth(u, nu[0])
        r = varcoef_relax_reference(u, kappa, f, A, boundary=cond, kappa_boundary=kbc)
        rc = restrict_reference(r)
        e = cycle(level + 1, torch.zeros_like(rc), rc, restrict_reference(kappa), hom)
        u = prolong_reference(e, boundary=hom, add=u)
        return smooth(u, nu[1])

    return cycle(0, u, f, kappa, bc)


def mgpcg_reference(u0: torch.Tensor, f: torch.Tensor, weights_per_level, bc, kappa=None, kappa_bc=None,
                    precond_dtype=None, nu=(2, 2), omega: float = 6.0 / 7.0, coarse_sweeps: int = 32, tol: float = 1e-8,
                    max_iters: int = 200, flexible: bool = True):
    """The algorithm of `models.StarPCG.solve` on gathered global (z, y, x) grids: conjugate gradients on
    `weights_per_level[0]` (under `bc`; the search direction under its homogeneous twin) preconditioned by one V-cycle
    from 0 (`mg_cycle_reference`, or `varcoef_mg_cycle_reference` with `kappa`) under the homogeneous conditions. The
    cycle runs in `precond_dtype` (None: f's): z = convert(cycle(0, convert(r, 1 / s)), s) with s = ||r||2 and, for
    VarCoefWeights, the coefficient `convert_reference(kappa, 1, precond_dtype)`. flexible: beta = -alpha (z . Ap) /
    rho_old (Polak-Ribiere), else rho / rho_old. Fields are in f's dtype through `axpby_reference`; every scalar is a
    torch double sum. Returns (u, history), history the recursive ||r||2 / ||f||2 after every iteration. The yardstick
    of the convergence tests; not bitwise (the solver's reductions sum in another order)."""
    from .. import _C
    from ..models.star_cg import _conditions
    from ..models.varcoef_model import kappa_conditions

    A = weights_per_level[0]
    od = f.dtype
    pd = od if precond_dtype is None else precond_dtype
    hom = None if bc is None else _conditions(bc, True)
    varcoef = isinstance(A, _C.VarCoefWeights)
    if varcoef:
        kbc = None if bc is None else kappa_conditions(bc, kappa_bc)
        kp = convert_reference(kappa, 1.0, pd)

    def apply(v, cond):
        if varcoef:
            return varcoef_step_reference(v, kappa, A, boundary=cond, kappa_boundary=kbc)
        step = box_step_reference if isinstance(A, _C.BoxWeights) else star_step_reference
        return step(v, A, boundary=cond)

    def dot(a, b):
        return float((a.double() * b.double()).sum())

    def precondition(r, s):
        g = convert_reference(r, 1.0 / s, pd)
        if varcoef:
            e = varcoef_mg_cycle_reference(torch.zeros_like(g), g, kp, weights_per_level, hom, kappa_bc, nu, omega,
                                           coarse_sweeps)
        else:
            e = mg_cycle_reference(torch.zeros_like(g), g, weights_per_level, hom, nu, omega, coarse_sweeps)
        return convert_reference(e, s, od)

    history = []
    ff = dot(f, f)
    if ff == 0:
        return torch.zeros_like(f), history
    u = u0.clone()
    r = axpby_reference(1.0, f, -1.0, apply(u, bc))
    rr = dot(r, r)
    if max_iters <= 0 or math.sqrt(rr / ff) < tol:
        return u, history
    z = precondition(r, math.sqrt(rr))
    rho = dot(r, z)
    p = z.clone()
    while True:
        Ap = apply(p, hom)
        alpha = rho / dot(p, Ap)
        u = axpby_reference(1.0, u, alpha, p)
        r = axpby_reference(1.0, r, -alpha, Ap)
        rr = dot(r, r)
        history.append(math.sqrt(rr / ff))
        if len(history) >= max_iters or history[-1] < tol:
            return u, history
        z = precondition(r, math.sqrt(rr))
        rho_new = dot(r, z)
        beta = -alpha * dot(z, Ap) / rho if flexible else rho_new / rho
        p = axpby_reference(1.0, z, beta, p)
        rho = rho_new


__all__ = ["periodic_gather", "jacobi_spheres", "jacobi_step_reference", "astaroth_step_reference",
           "astaroth_init_reference", "star_step_reference", "box_step_reference", "varcoef_step_reference", "varcoef_relax_reference", "varcoef_mg_cycle_reference", "axpby_reference", "convert_reference", "mgpcg_reference", "restrict_reference", "prolong_reference", "mg_cycle_reference", "pad_reference", "boundary_fill_reference", "math"]
