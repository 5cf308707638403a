"""StarCG on 256^3 fp32, Helmholtz (I - Laplacian), all-Mirror walls: ms per iteration (tol = 0: every iteration runs)"""
import sys
import time

import torch

import stencil2_amd as st
from stencil2_amd.ops import star_weights

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
FC = st.FaceCondition
bc = st.BoundaryConditions()
for ax in range(3):
    bc.set_axis(ax, FC.mirror(), FC.mirror())
w = star_weights(1, 7.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])
m = st.StarCG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group())
gen = torch.Generator().manual_seed(5)
f = (torch.rand((n, n, n), generator=gen) * 2 - 1).cuda()
m.set_rhs(lambda gz, gy, gx: f[gz % n, gy % n, gx % n])
m.solve(tol=0.0, max_iters=3)  # warm-up
m.set_guess()
torch.cuda.synchronize()
t0 = time.perf_counter()
it, rel = m.solve(tol=0.0, max_iters=iters)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"starcg,n,{n},iters,{it},relres,{rel:.3e},ms_per_iter,{dt * 1e3 / it:.4f}")
