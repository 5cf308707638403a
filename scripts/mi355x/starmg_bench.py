"""StarMG on 256^3 fp32, -Laplacian (7 points) between AntiMirror walls: ms per V(2,2) cycle, the cycles and wall time
to tol = 1e-5, and the wall time of StarCG to the same tolerance on the same problem (reported, no conditions)"""
import sys
import time

import torch

import stencil2_amd as st
from stencil2_amd.ops import star_weights

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 10
tol = 1e-5
FC = st.FaceCondition
bc = st.BoundaryConditions()
for ax in range(3):
    bc.set_axis(ax, FC.antimirror(0.0), FC.antimirror(0.0))
w = star_weights(1, 6.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])
gen = torch.Generator().manual_seed(5)
f = (torch.rand((n, n, n), generator=gen) * 2 - 1).cuda()


def rhs(gz, gy, gx):
    return f[gz % n, gy % n, gx % n]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


mg = st.StarMG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group())
mg.set_rhs(rhs)
mg.solve(tol=0.0, max_cycles=2)  # warm-up
mg.set_guess()
_, dt = timed(lambda: [mg.cycle() for _ in range(cycles)])
print(f"starmg,n,{n},levels,{mg.levels},cycles,{cycles},ms_per_cycle,{dt * 1e3 / cycles:.4f}")
mg.set_guess()
(k, rel), dt = timed(lambda: mg.solve(tol=tol))
print(f"starmg_solve,n,{n},tol,{tol:g},cycles,{k},relres,{rel:.3e},ms,{dt * 1e3:.3f}")

cg = st.StarCG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group())
cg.set_rhs(rhs)
cg.solve(tol=0.0, max_iters=3)  # warm-up
cg.set_guess()
(it, rel), dt = timed(lambda: cg.solve(tol=tol, max_iters=5000))
print(f"starcg_solve,n,{n},tol,{tol:g},iters,{it},relres,{rel:.3e},ms,{dt * 1e3:.3f}")
