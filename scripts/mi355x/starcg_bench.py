"""StarCG on 256^3 fp32, all-Mirror walls: ms per iteration (tol = 0: every iteration runs) of Helmholtz (I - Laplacian)
as a radius-1 star, then of the variable-coefficient operator 1 - div(kappa grad), kappa in [0.5, 1.5), in the same run"""
import sys
import time

import torch

import stencil2_amd as st
from stencil2_amd.ops import operator_varcoef, star_weights

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
FC = st.FaceCondition
bc = st.BoundaryConditions()
for ax in range(3):
    bc.set_axis(ax, FC.mirror(), FC.mirror())
gen = torch.Generator().manual_seed(5)
f = (torch.rand((n, n, n), generator=gen) * 2 - 1).cuda()
kappa = (0.5 + torch.rand((n, n, n), generator=gen)).cuda()


def bench(name, w, **kw):
    m = st.StarCG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group(), **kw)
    m.set_rhs(lambda gz, gy, gx: f[gz % n, gy % n, gx % n])
    m.solve(tol=0.0, max_iters=3)  # warm-up
    m.set_guess()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it, rel = m.solve(tol=0.0, max_iters=iters)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{name},n,{n},iters,{it},relres,{rel:.3e},ms_per_iter,{dt * 1e3 / it:.4f}")


bench("starcg", star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]))
bench("starcg_varcoef", operator_varcoef(1.0), kappa=lambda gz, gy, gx: kappa[gz % n, gy % n, gx % n])
