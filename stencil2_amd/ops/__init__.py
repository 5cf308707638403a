"""Kernel entry points and pure-torch fp32/fp64 oracles (used by the numerics tests)."""
from .reference import (  # noqa: F401
    astaroth_init_reference,
    astaroth_step_reference,
    jacobi_spheres,
    jacobi_step_reference,
    periodic_gather,
    star_step_reference,
)
from .kernels import (  # noqa: F401
    field_reduce,
    field_reduce_launch_info,
    field_reduce_supported,
    star_apply,
    star_launch_info,
    star_supported,
    stencil7_apply,
    stencil7_apply_regions,
    stencil7_wrappable_axes,
    stencil7x2_apply,
    stencil7x2_apply_exterior,
    stencil7x2_apply_regions,
    stencil7x2_wrappable_axes,
    stencil7x2_launch_info,
    stencil7x2_supported,
    stencil7x3_apply,
    stencil7x3_launch_info,
    stencil7x3_supported,
)
from .star import (  # noqa: F401
    diffusion_star,
    laplacian_star,
    star_to_lists,
    star_weights,
)
