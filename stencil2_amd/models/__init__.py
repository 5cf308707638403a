"""Stencil applications (the reference's bin/jacobi3d.cu and bin/astaroth_sim.cu) as models."""
from .stencil_model import Jacobi3D, AstarothSim, StencilModel, weak_scaled_size  # noqa: F401
from .star_model import StarStencil3D  # noqa: F401
from .box_model import BoxStencil3D  # noqa: F401
from .varcoef_model import VarCoefStencil3D  # noqa: F401
