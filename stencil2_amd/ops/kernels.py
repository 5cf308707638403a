"""Thin wrappers over the native HIP kernels (csrc/src/kernels/*.hip)."""
from __future__ import annotations

from .. import _C


def _tune(tune):
    return tune if tune is not None else _C.StencilTune()


def stencil7_apply(dd, di: int, q: int, region, kind=_C.StencilKind.Jacobi, spheres: bool = True, stream: int = 0,
                   tune=None):
    """next(region) = 7-point stencil of curr for quantity q of local sub-domain di (HIP kernel on its GPU). `tune`
    (a StencilTune, default the default tune) selects the kernel instance: variant, ty, nw, zchunk, nontemporal,
    xcd_remap, alternate_z, and wrap (the axes read periodically in-kernel: `stencil7_wrappable_axes`)."""
    native = getattr(dd, "native", dd)
    _C.stencil7_apply(native, di, q, region, kind, spheres, stream, _tune(tune))


def stencil7_wrappable_axes(dd, di: int, q: int) -> int:
    """mask (1 = x, 2 = y, 4 = z) of the axes `stencil7_apply` / `stencil7_apply_regions` can wrap in-kernel"""
    return _C.stencil7_wrappable_axes(getattr(dd, "native", dd), di, q)


def stencil7_apply_regions(dd, di: int, q: int, regions, kind=_C.StencilKind.Jacobi, spheres: bool = True,
                           stream: int = 0, tune=None):
    """One single step on every region of `regions` (Rect3 in global coordinates, each inside the compute region) in
    one call: the exterior slabs of an overlapped step. Of `tune` only `wrap` matters on the device."""
    native = getattr(dd, "native", dd)
    _C.stencil7_apply_regions(native, di, q, list(regions), kind, spheres, stream, _tune(tune))


def stencil7x2_wrappable_axes(dd, di: int, q: int, x2row: int = 1) -> int:
    """mask (1 = x, 2 = y, 4 = z) of the axes the fused-pair kernels can wrap in-kernel (x2row as StencilTune.x2row)"""
    return _C.stencil7x2_wrappable_axes(getattr(dd, "native", dd), di, q, x2row)


def stencil7x2_apply_regions(dd, di: int, q: int, regions, kind=_C.StencilKind.Jacobi, spheres: bool = True,
                             stream: int = 0, wrap: int = 0):
    """next = S(S(curr)) on every region of `regions`, one thread per cell (the thick exterior slabs of an overlapped
    fused pair); `wrap`: the axes read periodically in-kernel."""
    native = getattr(dd, "native", dd)
    _C.stencil7x2_apply_regions(native, di, q, list(regions), kind, spheres, stream, wrap)


def stencil7x2_apply_exterior(dd, di: int, q: int, interior, kind=_C.StencilKind.Jacobi, spheres: bool = True,
                              stream: int = 0, tune=None):
    """next = S(S(curr)) on the compute region minus `interior` (the exterior of an overlapped fused pair): slabs up to
    4 cells thick by the thin-slab kernels, thicker ones one thread per cell."""
    native = getattr(dd, "native", dd)
    _C.stencil7x2_apply_exterior(native, di, q, interior, kind, spheres, stream, _tune(tune))


def stencil7x2_supported(dd, di: int, q: int) -> bool:
    """True when the fused two-step kernel can run on quantity q of local sub-domain di: a device fp32/fp64 quantity,
    face radii >= 2 (edges >= 1) and the aligned row layout."""
    return _C.stencil7x2_supported(getattr(dd, "native", dd), di, q)


def stencil7x2_apply(dd, di: int, q: int, region, kind=_C.StencilKind.Jacobi, spheres: bool = True, stream: int = 0,
                     tune=None):
    """next(region) = S(S(curr)) -- two fused 7-point steps (temporal blocking), bitwise equal to two single steps --
    for quantity q of local sub-domain di. The depth-2 face and depth-1 edge halos of curr must be valid (exchange()
    first); with `tune.wrap` set, the axes in that mask are read periodically in-kernel instead (the region must then
    span them). One read and one write of the field per two steps (csrc/src/kernels/stencil7x2.hip)."""
    native = getattr(dd, "native", dd)
    _C.stencil7x2_apply(native, di, q, region, kind, spheres, stream, tune if tune is not None else _C.StencilTune())


def stencil7x2_launch_info(dd, di: int, q: int, region=None, kind=_C.StencilKind.Jacobi, spheres: bool = True,
                           tune=None) -> dict:
    """What `stencil7x2_apply` would launch for these arguments (nothing is launched; the same refusals raise;
    `region` defaults to the sub-domain's compute region): `form` ("row": whole 512-cell periodic rows, "ragged2" /
    "ragged3": periodic rows of 257-511 / 513-768 cells, "tail": 769-832 cells, "col2": two-chunk columns, "column":
    the one-chunk column kernel; `_C.stencil7x2_form`), `wrap_variant` (the kernel's in-kernel wrap: 0 none, 1 y / z,
    2 x too), `cols` (block columns), `slots` (resident blocks: the occupancy query less the share of
    `tune.reserveCUs`) and the schedule `seg` (0 fixed z chunks, 1 balanced split, 2 lockstep parts plus second
    segments, 3 lockstep rounds), `parts`, `rounds`, `blocks`, `zchunk`, `gz` (`_C.stencil7x2_schedule`)."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return _C.stencil7x2_launch_info(native, di, q, region, kind, spheres, tune if tune is not None else _C.StencilTune())


def stencil7x3_supported(dd, di: int, q: int, tune=None) -> bool:
    """True when the fused three-step kernel can sweep quantity q of local sub-domain di: a device fp32/fp64 quantity
    in the aligned row layout with at least 3 x 3 x 16 cells, face radii >= 3 (edges and corners >= 1) on every axis
    that `tune.wrap` does not read in-kernel, and an x extent the kernel's columns cover: with x wrapped in-kernel
    (`tune.wrap & 1`) fp32 rows of exactly 512 cells; with x read from halos any row whose last column of 512 fp32 /
    256 fp64 cells holds at most 509 / 253 cells (a whole column, or a partial one that leaves room for the 3 halo
    cells; rows ending 1 or 2 cells short of a whole column keep the fused pairs)."""
    return _C.stencil7x3_supported(getattr(dd, "native", dd), di, q, tune if tune is not None else _C.StencilTune())


def stencil7x3_launch_info(dd, di: int, q: int, kind=_C.StencilKind.Jacobi, spheres: bool = True, tune=None) -> dict:
    """What `stencil7x3_apply` would launch for quantity q of local sub-domain di with this kind, spheres and tune
    (nothing is launched): `supported`, `form` ("wrap": whole rows wrapped in-kernel, "xh": columns with x halos),
    `ragged` (a partial last column), `cols` ((row group, column) pairs), `slots` (resident blocks: the occupancy query
    less the share of `tune.reserveCUs`), and the schedule `seg` (1 balanced split, 2 lockstep parts plus second
    segments, 3 lockstep rounds), `parts`, `blocks`, `rounds`. The schedule is `_C.stencil7x3_schedule`'s, refined by
    the host plan for seg 2."""
    native = getattr(dd, "native", dd)
    return _C.stencil7x3_launch_info(native, di, q, kind, spheres, tune if tune is not None else _C.StencilTune())


def stencil7x3_apply(dd, di: int, q: int, kind=_C.StencilKind.Jacobi, spheres: bool = True, stream: int = 0,
                     tune=None) -> bool:
    """next = S(S(S(curr))) on the whole compute region of local sub-domain di -- three fused 7-point steps (deeper
    temporal blocking), bitwise equal to three single steps -- for quantity q. Returns False without launching
    where `stencil7x3_supported` refuses. The halos of curr that must be valid (exchange() first): depth 3 on the
    faces, and depth >= 1 on every edge and corner whose axes are all read from halos; the axes set in `tune.wrap`
    are read periodically in-kernel instead and need no halo. One read and one write of the field per three steps;
    only cells of the compute region are written (csrc/src/kernels/stencil7x3.hip)."""
    native = getattr(dd, "native", dd)
    return _C.stencil7x3_apply(native, di, q, kind, spheres, stream, tune if tune is not None else _C.StencilTune())


def _reduce_args(dd, di, q, other, region):
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return native, (-1 if other is None else int(other)), region


def field_reduce(dd, di: int, q: int, other=None, curr: bool = True, other_curr: bool = False, region=None,
                 stream: int = 0, max_blocks: int = 0):
    """FieldStats (count, nonfinite, sum, sum_abs, sum_sq, min, max, dot; l1, l2, linf) of quantity q of local
    sub-domain di over `region` (global coordinates, default the sub-domain's compute region); no communication.
    One operand: e = double(q); with `other`: e = double(q) - double(other) and dot = sum of q * other. `curr` /
    `other_curr` pick each operand's curr or next buffer. Blocking: enqueued on `stream` and waited for. Accumulation
    is in double, without atomics, in an order fixed by the layout, the region and the grid (`max_blocks`: 0 = one
    round of resident blocks, else exactly that many), so the same call returns the same bits every time
    (csrc/src/kernels/field_reduce.hip)."""
    native, qb, region = _reduce_args(dd, di, q, other, region)
    return _C.field_reduce(native, di, q, curr, qb, other_curr, region, stream, max_blocks)


def field_reduce_launch_info(dd, di: int, q: int, other=None, curr: bool = True, other_curr: bool = False, region=None,
                             max_blocks: int = 0) -> dict:
    """What `field_reduce` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the row kernel of the aligned vector layout, "generic": one thread per cell, "host", "none": empty
    region), `blocks` of the launch and `items`, the (row, plane) pairs of the region."""
    native, qb, region = _reduce_args(dd, di, q, other, region)
    return _C.field_reduce_launch_info(native, di, q, curr, qb, other_curr, region, max_blocks)


def field_reduce_supported(dd, di: int, q: int, other=None) -> bool:
    """True when `field_reduce` takes quantity q (and `other`) of local sub-domain di: fp32 / fp64 quantities (or
    opaque 4- / 8-byte elements) of the same element size."""
    return _C.field_reduce_supported(getattr(dd, "native", dd), di, q, -1 if other is None else int(other))


def _axpby_args(dd, di, y, region):
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return native, (-1 if y is None else int(y)), region


def field_axpby(dd, di: int, dst: int, a: float, x: int, b: float = 0.0, y=None, dst_curr: bool = True,
                x_curr: bool = True, y_curr: bool = True, region=None, stream: int = 0, stats: bool = False,
                max_blocks: int = 0, nontemporal: bool = False):
    """dst(region) = a * x (y None) or a * x + b * y for quantities of local sub-domain di; `*_curr` pick each
    operand's curr or next buffer and `region` (global coordinates) defaults to the sub-domain's compute region. a and
    b are converted to the element type once; every product and the sum is its own rounding in that type, so the
    result is bitwise equal to `axpby_reference`. dst may alias x and / or y. Only cells of the region are written, so
    the halos of dst are stale afterwards. Asynchronous on `stream` and returns None; with `stats` it waits for the
    stream and returns the FieldStats of the stored values, accumulated in the same pass as `field_reduce` would
    (dot = 0). `max_blocks`: 0 = one round of resident blocks, else exactly that many; `nontemporal`: nt-hinted 16-B
    stores (csrc/src/kernels/field_axpby.hip)."""
    native, qy, region = _axpby_args(dd, di, y, region)
    return _C.field_axpby(native, di, int(dst), bool(dst_curr), float(a), int(x), bool(x_curr), float(b), qy,
                          bool(y_curr), region, stream, bool(stats), max_blocks, bool(nontemporal))


def field_axpby_launch_info(dd, di: int, dst: int, a: float, x: int, b: float = 0.0, y=None, dst_curr: bool = True,
                            x_curr: bool = True, y_curr: bool = True, region=None, stats: bool = False,
                            max_blocks: int = 0, nontemporal: bool = False) -> dict:
    """What `field_axpby` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the row kernel of the aligned vector layout, "generic": one thread per cell, "host", "none": empty
    region), `blocks` of the launch and `items`, the (row, plane) pairs of the region."""
    native, qy, region = _axpby_args(dd, di, y, region)
    return _C.field_axpby_launch_info(native, di, int(dst), bool(dst_curr), float(a), int(x), bool(x_curr), float(b),
                                      qy, bool(y_curr), region, bool(stats), max_blocks, bool(nontemporal))


def field_axpby_supported(dd, di: int, dst: int, x: int, y=None) -> bool:
    """True when `field_axpby` takes these quantities of local sub-domain di: fp32 / fp64 quantities (or opaque 4- /
    8-byte elements) of one element size and row pitch."""
    return _C.field_axpby_supported(getattr(dd, "native", dd), di, int(dst), int(x), -1 if y is None else int(y))


def _convert_args(src_dd, dst_dd, di, region):
    src, dst = getattr(src_dd, "native", src_dd), getattr(dst_dd, "native", dst_dd)
    if region is None:
        region = dst.domain(di).get_compute_region()
    return src, dst, region


def field_convert(src_dd, dst_dd, di: int, src: int, dst: int, scale: float = 1.0, src_curr: bool = True,
                  dst_curr: bool = True, region=None, stream: int = 0, stats: bool = False, max_blocks: int = 0):
    """dst(region) = T_dst(scale * double(src)): quantity `src` of local sub-domain di of `src_dd` into quantity `dst`
    of sub-domain di of `dst_dd`, fp32 or fp64 on each side. One product in double and one conversion to the
    destination type, so the result is bitwise equal to `convert_reference`; scale = 1 is an exact cast. The two
    domains (which may be the same object) are on one backend and device and give sub-domain di the same compute
    region; radii, pitches and padding may differ. `*_curr` pick each side's curr or next buffer and `region` (global
    coordinates) defaults to the compute region. Only cells of the region are written, so the halos of dst are stale
    afterwards. Asynchronous on `stream` and returns None; with `stats` it waits for the stream and returns the
    FieldStats of the stored values from the same pass, as `field_axpby` does. `max_blocks`: 0 = one round of
    resident blocks, else exactly that many (csrc/src/kernels/field_convert.hip)."""
    s, d, region = _convert_args(src_dd, dst_dd, di, region)
    return _C.field_convert(s, d, di, int(src), bool(src_curr), int(dst), bool(dst_curr), float(scale), region, stream,
                            bool(stats), max_blocks)


def field_convert_launch_info(src_dd, dst_dd, di: int, src: int, dst: int, scale: float = 1.0, src_curr: bool = True,
                              dst_curr: bool = True, region=None, stats: bool = False, max_blocks: int = 0) -> dict:
    """What `field_convert` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the row kernel when both sides are in the aligned vector layout, "generic": one thread per cell, "host",
    "none": empty region), `blocks` of the launch and `items`, the (row, plane) pairs of the region."""
    s, d, region = _convert_args(src_dd, dst_dd, di, region)
    return _C.field_convert_launch_info(s, d, di, int(src), bool(src_curr), int(dst), bool(dst_curr), float(scale),
                                        region, bool(stats), max_blocks)


def field_convert_supported(src_dd, dst_dd, di: int, src: int, dst: int) -> bool:
    """True when `field_convert` takes quantity `src` of `src_dd` and `dst` of `dst_dd` for local sub-domain di: fp32 /
    fp64 quantities (or opaque 4- / 8-byte elements) of realized domains on one backend and device with the same
    compute region."""
    return _C.field_convert_supported(getattr(src_dd, "native", src_dd), getattr(dst_dd, "native", dst_dd), di,
                                      int(src), int(dst))


def _fill_args(dd, q, bc):
    """(native, quantities, conditions): q None = every quantity whose conditions fill a face, as apply_boundary()"""
    native = getattr(dd, "native", dd)
    if q is None:
        qs = list(range(native.domain(0).num_data()))
    else:
        qs = [int(v) for v in q] if isinstance(q, (list, tuple)) else [int(q)]
    if bc is None:
        bcs = [native.boundary_conditions(v) for v in qs]
    else:
        bcs = list(bc) if isinstance(bc, (list, tuple)) else [bc] * len(qs)
    return native, qs, bcs


def boundary_apply(dd, di: int, q, bc=None, curr: bool = True, stream: int = 0):
    """Fill the ghost cells of quantity q (an index, a list, or None = every quantity) of local sub-domain di beyond
    the non-periodic faces of the global grid under `bc` (_C.BoundaryConditions, default the domain's conditions for
    q): Constant faces T(v), Mirror faces the mirror cell, AntiMirror faces T(2 v) - mirror cell, Open faces left
    alone; edges and corners resolve z, then y, then x (ops.boundary_fill_reference). One launch for the whole list,
    asynchronous on `stream`; only ghost cells are written and only other cells are read. It belongs after the
    exchange has landed (csrc/src/kernels/boundary_fill.hip)."""
    native, qs, bcs = _fill_args(dd, q, bc)
    _C.boundary_fill(native, di, qs, bcs, curr, stream)


def boundary_launch_info(dd, di: int, q=None, bc=None) -> dict:
    """What `boundary_apply` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the row / column kernel of the aligned vector layout, "generic": one thread per ghost cell, "host",
    "none": the sub-domain touches no face that is filled), `boxes` (disjoint boxes of ghost cells over all
    quantities), `blocks` and `launches` (one per 16 quantities)."""
    native, qs, bcs = _fill_args(dd, q, bc)
    return _C.boundary_fill_launch_info(native, di, qs, bcs)


def boundary_supported(dd, di: int, q: int, bc=None) -> bool:
    """True when `boundary_apply` takes quantity q of local sub-domain di under `bc`: an fp32 / fp64 quantity (or
    opaque 4- / 8-byte elements) whose extent along every Mirror / AntiMirror face the sub-domain touches is at least
    that side's face radius."""
    native, qs, bcs = _fill_args(dd, q, bc)
    return _C.boundary_fill_supported(native, di, qs[0], bcs[0])


def star_supported(dd, di: int, q: int, weights) -> bool:
    """True when `star_apply` can run `weights` on quantity q of local sub-domain di: an fp32 / fp64 quantity (or
    opaque 4- / 8-byte elements), radius 1..3 and all six face radii of the domain >= that radius."""
    return _C.stencil_star_supported(getattr(dd, "native", dd), di, q, weights)


def star_apply(dd, di: int, q: int, weights, region=None, stream: int = 0, tune=None):
    """next(region) = weighted star stencil of curr (`weights`: ops.star_weights / laplacian_star / diffusion_star)
    for quantity q of local sub-domain di; `region` (global coordinates) defaults to the sub-domain's compute region
    and only its cells are written. The face halos of curr must be valid to depth `weights.radius` (exchange() first).
    Every product and sum is its own rounding in the quantity's type, in the order of `star_step_reference`, so the
    result is bitwise equal to it (csrc/src/kernels/stencil_star.hip)."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    _C.stencil_star_apply(native, di, q, region, weights, stream, _tune(tune))


def star_launch_info(dd, di: int, q: int, weights, region=None, tune=None) -> dict:
    """What `star_apply` would run for these arguments (nothing is launched; the same refusals raise): `path` ("fast":
    the z-march kernel of the aligned vector layout, "generic": one thread per cell, "host", "none": empty region) and
    the z-march launch `zchunk` (planes per block), `zchunks`, `blocks`."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return _C.stencil_star_launch_info(native, di, q, region, weights, _tune(tune))


def box_supported(dd, di: int, q: int) -> bool:
    """True when `box_apply` can run on quantity q of local sub-domain di: an fp32 / fp64 quantity (or opaque 4- /
    8-byte elements) and all 26 direction radii of the domain >= 1 (a 19-point box still needs the corners exchanged:
    zero weights are multiplied like any other)."""
    return _C.stencil_box_supported(getattr(dd, "native", dd), di, q)


def box_apply(dd, di: int, q: int, weights, region=None, stream: int = 0, tune=None):
    """next(region) = weighted 27-point box stencil of curr (`weights`: ops.box_weights / laplacian_box /
    diffusion_box / smoothing_box) for quantity q of local sub-domain di; `region` (global coordinates) defaults to
    the sub-domain's compute region and only its cells are written. The face, edge and corner halos of curr must be
    valid to depth 1 (exchange() first). Every product and sum is its own rounding in the quantity's type, in the
    order of `box_step_reference` (dz slowest, dx fastest, from (-1, -1, -1)), so the result is bitwise equal to it.
    Of `tune`: zchunk, nontemporal, xcd_remap; alternate_z is ignored (every z chunk marches upwards, because the sum
    takes dz = -1 first) and wrap != 0 is refused (csrc/src/kernels/stencil_box.hip)."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    _C.stencil_box_apply(native, di, q, region, weights, stream, _tune(tune))


def box_launch_info(dd, di: int, q: int, weights, region=None, tune=None) -> dict:
    """What `box_apply` would run for these arguments (nothing is launched; the same refusals raise): `path` ("fast":
    the z-march kernel of the aligned vector layout, "generic": one thread per cell, "host", "none": empty region) and
    the z-march launch `zchunk` (planes per block), `zchunks`, `blocks`."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return _C.stencil_box_launch_info(native, di, q, region, weights, _tune(tune))


def varcoef_supported(dd, di: int, q: int, kappa: int) -> bool:
    """True when `varcoef_apply` can run on quantity q with the coefficient quantity `kappa` of local sub-domain di:
    fp32 / fp64 quantities (or opaque 4- / 8-byte elements) of one element size and row pitch, and all six face radii
    of the domain >= 1."""
    return _C.stencil_varcoef_supported(getattr(dd, "native", dd), di, int(q), int(kappa))


def varcoef_apply(dd, di: int, q: int, kappa: int, w, region=None, stream: int = 0, tune=None):
    """next(q)(region) = w.shift * u + sum over the six faces of w.h[axis] * (kappa(c) + kappa(n)) * (u(n) - u(c)) with
    u = curr(q) and kappa = curr(kappa) of local sub-domain di (`w`: ops.varcoef_weights / diffusion_varcoef /
    operator_varcoef); `region` (global coordinates) defaults to the sub-domain's compute region and only its cells of
    next(q) are written, so kappa == q is allowed. The face halos of both curr buffers must be valid to depth 1
    (exchange() first). Every sum, difference and product is its own rounding in the quantities' type, in the order of
    `varcoef_step_reference`, so the result is bitwise equal to it. Of `tune`: zchunk, nontemporal, xcd_remap,
    alternate_z; wrap != 0 is refused (csrc/src/kernels/stencil_varcoef.hip)."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    _C.stencil_varcoef_apply(native, di, int(q), int(kappa), region, w, stream, _tune(tune))


def varcoef_launch_info(dd, di: int, q: int, kappa: int, w, region=None, tune=None) -> dict:
    """What `varcoef_apply` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the z-march kernel of the aligned vector layout, "generic": one thread per cell, "host", "none": empty
    region) and the z-march launch `zchunk` (planes per block), `zchunks`, `blocks`."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return _C.stencil_varcoef_launch_info(native, di, int(q), int(kappa), region, w, _tune(tune))


def _relax_dst(q, dst):
    return int(q) if dst is None else int(dst)


def varcoef_relax_supported(dd, di: int, q: int, kappa: int, f: int, dst=None) -> bool:
    """True when `varcoef_relax` can run on quantity q with the coefficient `kappa`, the right-hand side `f` and the
    destination quantity `dst` (default q) of local sub-domain di: fp32 / fp64 quantities (or opaque 4- / 8-byte
    elements) of one element size and row pitch, and all six face radii of the domain >= 1."""
    return _C.stencil_varcoef_relax_supported(getattr(dd, "native", dd), di, int(q), int(kappa), int(f),
                                              _relax_dst(q, dst))


def varcoef_relax(dd, di: int, q: int, kappa: int, f: int, w, omega=None, dst=None, dst_curr: bool = False, region=None,
                  stream: int = 0, tune=None):
    """One pass over u = curr(q), curr(kappa) and curr(f) of local sub-domain di with A the operator of
    `varcoef_apply` for `w`: omega=None stores the residual f - A u, otherwise the damped-Jacobi update
    u + omega * ((f - A u) / diag(A)), diag(A) = w.shift - sum over the six faces of w.h[axis] * (kappa(c) + kappa(n)).
    The destination is the next (or, with dst_curr, the curr) buffer of quantity `dst` (default q, so the default
    writes next(q)); only its cells of `region` (default the compute region) are written. curr(q) and curr(kappa)
    are refused as destination, curr(f) is allowed. The face halos of curr(q) and curr(kappa) must be valid to depth 1.
    Every sum, difference, product and quotient is its own rounding in the quantities' type, in the order of
    `varcoef_relax_reference`, so the result is bitwise equal to it (a zero diagonal gives inf / NaN). `tune` as for
    `varcoef_apply` (csrc/src/kernels/stencil_varcoef_relax.hip)."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    _C.stencil_varcoef_relax(native, di, int(q), int(kappa), int(f), _relax_dst(q, dst), bool(dst_curr), region, w,
                             omega is not None, 1.0 if omega is None else float(omega), stream, _tune(tune))


def varcoef_relax_launch_info(dd, di: int, q: int, kappa: int, f: int, w, omega=None, dst=None, dst_curr: bool = False,
                              region=None, tune=None) -> dict:
    """What `varcoef_relax` would run for these arguments (nothing is launched; the same refusals raise): `path`,
    `zchunk`, `zchunks`, `blocks` as `varcoef_launch_info`."""
    native = getattr(dd, "native", dd)
    if region is None:
        region = native.domain(di).get_compute_region()
    return _C.stencil_varcoef_relax_launch_info(native, di, int(q), int(kappa), int(f), _relax_dst(q, dst),
                                                bool(dst_curr), region, w, omega is not None, _tune(tune))


def _native(dd):
    return getattr(dd, "native", dd)


def _sub_region(native, di):
    """the compute region of local sub-domain di, the default region of a grid transfer"""
    n = native.num_domains()
    if not 0 <= di < n:
        raise IndexError(f"grid transfer: no local sub-domain {di} ({n} realized; an unrealized domain has none)")
    return native.domain(di).get_compute_region()


def grid_transfer_supported(fine_dd, coarse_dd, di: int, qf: int, qc: int) -> bool:
    """True when `restrict_apply` / `prolong_apply` take quantity qf of local sub-domain di of `fine_dd` and qc of the
    same sub-domain of `coarse_dd`: fp32 / fp64 quantities (or opaque 4- / 8-byte elements) of one element size, both
    domains realized, the coarse sub-domain the factor-2 image of the fine one (even origin and size, halved) on the
    same device and backend. Prolongation also needs every coarse direction radius >= 1."""
    return _C.grid_transfer_supported(_native(fine_dd), _native(coarse_dd), di, int(qf), int(qc))


def restrict_apply(fine_dd, coarse_dd, di: int, src: int, dst: int, src_curr: bool = True, dst_curr: bool = True,
                   region=None, stream: int = 0):
    """coarse dst(region) = R fine src between local sub-domain di of the two domains: cell-centred full weighting, the
    mean of the 8 fine cells under a coarse cell summed along x, then y, then z, every sum rounded on its own in the
    quantities' type, so the result is bitwise equal to `restrict_reference`. `region` (global coordinates of the
    coarse grid) defaults to the coarse sub-domain's compute region; only its cells are written and no halo is read.
    Asynchronous on `stream` (csrc/src/kernels/grid_transfer.hip)."""
    fine, coarse = _native(fine_dd), _native(coarse_dd)
    if region is None:
        region = _sub_region(coarse, di)
    _C.grid_restrict(fine, coarse, di, int(src), bool(src_curr), int(dst), bool(dst_curr), region, stream)


def restrict_launch_info(fine_dd, coarse_dd, di: int, src: int, dst: int, src_curr: bool = True, dst_curr: bool = True,
                         region=None) -> dict:
    """What `restrict_apply` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the chunk kernel of the aligned vector layout, "generic": one thread per coarse cell, "host", "none":
    empty region), `blocks` of the launch and `items`, the coarse (row, plane) pairs of the region."""
    fine, coarse = _native(fine_dd), _native(coarse_dd)
    if region is None:
        region = _sub_region(coarse, di)
    return _C.grid_restrict_launch_info(fine, coarse, di, int(src), bool(src_curr), int(dst), bool(dst_curr), region)


def prolong_apply(coarse_dd, fine_dd, di: int, src: int, dst: int, add=None, src_curr: bool = True,
                  dst_curr: bool = True, add_curr: bool = True, region=None, stream: int = 0, zchunk: int = 0):
    """fine dst(region) = P coarse src, or with `add` (a quantity of the fine domain, possibly dst itself: the
    correction u <- u + P e) add + P coarse src, between local sub-domain di of the two domains. P is trilinear
    (weights 3/4 and 1/4 per axis), evaluated along x, then y, then z with every product and sum rounded on its own,
    so the result is bitwise equal to `prolong_reference`. It reads one cell into the coarse halos in all 26
    directions: exchange the coarse domain and `apply_boundary` first. `region` (global coordinates of the fine grid)
    defaults to the fine sub-domain's compute region; only its cells are written. `zchunk`: the coarse planes a wave
    of the chunk kernel marches (0: chosen by the launch). Asynchronous on `stream` (csrc/src/kernels/grid_transfer.hip)."""
    coarse, fine = _native(coarse_dd), _native(fine_dd)
    if region is None:
        region = _sub_region(fine, di)
    _C.grid_prolong(coarse, fine, di, int(src), bool(src_curr), int(dst), bool(dst_curr),
                    -1 if add is None else int(add), bool(add_curr), region, stream, int(zchunk))


def prolong_launch_info(coarse_dd, fine_dd, di: int, src: int, dst: int, add=None, src_curr: bool = True,
                        dst_curr: bool = True, add_curr: bool = True, region=None, zchunk: int = 0) -> dict:
    """What `prolong_apply` would run for these arguments (nothing is launched; the same refusals raise): `path`
    ("fast": the z-march chunk kernel of the aligned vector layout, "generic": one thread per fine cell, "host",
    "none": empty region), `blocks`, `items` ((64 fine chunks, coarse row, z chunk) triples, one wave each) and `zchunk`
    (coarse planes per item)."""
    coarse, fine = _native(coarse_dd), _native(fine_dd)
    if region is None:
        region = _sub_region(fine, di)
    return _C.grid_prolong_launch_info(coarse, fine, di, int(src), bool(src_curr), int(dst), bool(dst_curr),
                                       -1 if add is None else int(add), bool(add_curr), region, int(zchunk))
