"""StarMG on 256^3 fp32, -Laplacian (7 points) between AntiMirror walls: ms per V(2,2) cycle, the cycles and wall time
to tol = 1e-5, and the wall time of StarCG to the same tolerance on the same problem (reported, no conditions).
--varcoef [--sigma S]: the same for S - div(kappa grad), S = 1 by default, with a seeded kappa in [0.5, 1.5)
(ops.operator_varcoef(S), the fused ops.varcoef_relax smoother); the output lines then start with "varcoef_"
("varcoef_sigmaS_" for another S)."""
import sys
import time

import torch

import stencil2_amd as st
from stencil2_amd.ops import operator_varcoef, star_weights

args = list(sys.argv[1:])
varcoef = "--varcoef" in args
if varcoef:
    args.remove("--varcoef")
sigma = 1.0
if "--sigma" in args:
    i = args.index("--sigma")
    sigma = float(args[i + 1])
    del args[i:i + 2]
n = int(args[0]) if len(args) > 0 else 256
cycles = int(args[1]) if len(args) > 1 else 10
tol = 1e-5
FC = st.FaceCondition
bc = st.BoundaryConditions()
for ax in range(3):
    bc.set_axis(ax, FC.antimirror(0.0), FC.antimirror(0.0))
w = operator_varcoef(sigma) if varcoef else star_weights(1, 6.0, [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0])
gen = torch.Generator().manual_seed(5)
f = (torch.rand((n, n, n), generator=gen) * 2 - 1).cuda()
kappa = (0.5 + torch.rand((n, n, n), generator=torch.Generator().manual_seed(23))).cuda() if varcoef else None
tag = ("varcoef_" if sigma == 1.0 else f"varcoef_sigma{sigma:g}_") if varcoef else ""


def rhs(gz, gy, gx):
    return f[gz % n, gy % n, gx % n]


def coef(gz, gy, gx):
    return kappa[gz % n, gy % n, gx % n]


kw = dict(kappa=coef) if varcoef else {}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


mg = st.StarMG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group(), **kw)
mg.set_rhs(rhs)
mg.solve(tol=0.0, max_cycles=2)  # warm-up
mg.set_guess()
_, dt = timed(lambda: [mg.cycle() for _ in range(cycles)])
print(f"{tag}starmg,n,{n},levels,{mg.levels},cycles,{cycles},ms_per_cycle,{dt * 1e3 / cycles:.4f}")
mg.set_guess()
(k, rel), dt = timed(lambda: mg.solve(tol=tol))
print(f"{tag}starmg_solve,n,{n},tol,{tol:g},cycles,{k},relres,{rel:.3e},ms,{dt * 1e3:.3f}")

cg = st.StarCG((n, n, n), w, fp64=False, gpus=[0], boundary=bc, group=st.make_single_group(), **kw)
cg.set_rhs(rhs)
cg.solve(tol=0.0, max_iters=3)  # warm-up
cg.set_guess()
(it, rel), dt = timed(lambda: cg.solve(tol=tol, max_iters=5000))
print(f"{tag}starcg_solve,n,{n},tol,{tol:g},iters,{it},relres,{rel:.3e},ms,{dt * 1e3:.3f}")
