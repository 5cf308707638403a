"""field_convert and StarPCG on one MI355X.

1. field_convert at 512^3 (the second argument) in both directions between an fp32 and an fp64 quantity of one domain,
   against field_axpby copies (a = 1) of each type: ms per launch and bytes/s of all four (a cell moves 4 + 8 bytes in a
   conversion, 8 in an fp32 copy, 16 in an fp64 copy).
2. -div(kappa grad u) = f at 256^3 (the first argument) with kappa = 1 + 99 [x >= n / 2 and y >= n / 4], a Mirror wall
   at the low x face and AntiMirror walls elsewhere: iterations and wall time of StarCG (fp64), StarMG (fp32 to 1e-5,
   fp64 to 1e-10) and StarPCG (fp64 outside with an fp64 and with an fp32 cycle; fp32 outside and inside to 1e-5) to
   1e-5 and to 1e-10. Solvers that hit their iteration cap report the residual they reached.

Reported, no conditions: every line is a measurement."""
import sys
import time

import torch

import stencil2_amd as st
from stencil2_amd.ops import field_axpby, field_convert, field_convert_launch_info, operator_varcoef

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
nc = int(sys.argv[2]) if len(sys.argv) > 2 else 512
reps = 20
FC = st.FaceCondition


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


# ---- 1. field_convert against field_axpby copies ----
dd = st.DistributedDomain(nc, nc, nc, group=st.make_single_group())
dd.set_radius(st.Radius.face_edge_corner(1, 0, 0))
dd.set_gpus([0])
a32, b32 = dd.add_data("a32", torch.float32), dd.add_data("b32", torch.float32)
a64, b64 = dd.add_data("a64", torch.float64), dd.add_data("b64", torch.float64)
dd.realize()
gen = torch.Generator().manual_seed(5)
for q, dt in ((a32, torch.float32), (a64, torch.float64)):
    dd.curr(0, q).copy_(torch.rand(dd.curr(0, q).shape, generator=gen, dtype=dt))
cells = nc ** 3
launches = {
    "convert_fp32_to_fp64": (12, lambda: field_convert(dd, dd, 0, a32, b64)),
    "convert_fp64_to_fp32": (12, lambda: field_convert(dd, dd, 0, a64, b32)),
    "convert_fp32_to_fp32": (8, lambda: field_convert(dd, dd, 0, a32, b32)),
    "convert_fp64_to_fp64": (16, lambda: field_convert(dd, dd, 0, a64, b64)),
    "axpby_copy_fp32": (8, lambda: field_axpby(dd, 0, b32, 1.0, a32)),
    "axpby_copy_fp64": (16, lambda: field_axpby(dd, 0, b64, 1.0, a64)),
    "convert_fp64_to_fp32_stats": (12, lambda: field_convert(dd, dd, 0, a64, b32, stats=True)),
    "axpby_copy_fp32_stats": (8, lambda: field_axpby(dd, 0, b32, 1.0, a32, stats=True)),
}
print(f"convert_info,n,{nc},{field_convert_launch_info(dd, dd, 0, a32, b64)}")
for name, (bpc, fn) in launches.items():
    for _ in range(3):
        fn()
    best = min(timed(lambda: [fn() for _ in range(reps)])[1] for _ in range(3)) / reps
    print(f"{name},n,{nc},ms,{best * 1e3:.4f},GB_per_s,{cells * bpc / best / 1e9:.1f}")
del dd
torch.cuda.empty_cache()

# ---- 2. the solvers ----
bc = st.BoundaryConditions()
bc.set_axis(0, FC.mirror(), FC.antimirror(0.0))
for ax in (1, 2):
    bc.set_axis(ax, FC.antimirror(0.0), FC.antimirror(0.0))
w = operator_varcoef(0.0)
f = torch.randn((n, n, n), generator=torch.Generator().manual_seed(1301), dtype=torch.float64).cuda()


def rhs(gz, gy, gx):
    return f[gz % n, gy % n, gx % n]


def coef(gz, gy, gx):
    return 1.0 + 99.0 * ((gx >= n // 2) & (gy >= n // 4) & (gz >= 0)).double()


kw = dict(gpus=[0], boundary=bc, group=st.make_single_group(), kappa=coef)


def run(name, make, solve, tols):
    m = make()
    m.set_rhs(rhs)
    solve(m, 0.0, 2)  # warm-up
    for tol in tols:
        m.set_guess()
        (k, rel), dt = timed(lambda: solve(m, tol, None))
        print(f"{name},n,{n},tol,{tol:g},iters,{k},relres,{rel:.3e},ms,{dt * 1e3:.3f},ms_per_iter,{dt * 1e3 / max(k, 1):.4f}")


def cg_solve(m, tol, cap):
    return m.solve(tol=tol, max_iters=cap if cap is not None else 20000)


def mg_solve(m, tol, cap):
    return m.solve(tol=tol, max_cycles=cap if cap is not None else 60)


def pcg_solve(m, tol, cap):
    return m.solve(tol=tol, max_iters=cap if cap is not None else 200)


run("starpcg_fp64_cycle_fp64", lambda: st.StarPCG((n, n, n), w, fp64=True, precond_fp64=True, **kw), pcg_solve, (1e-5, 1e-10))
run("starpcg_fp64_cycle_fp32", lambda: st.StarPCG((n, n, n), w, fp64=True, precond_fp64=False, **kw), pcg_solve, (1e-5, 1e-10))
run("starpcg_fp32_cycle_fp32", lambda: st.StarPCG((n, n, n), w, fp64=False, precond_fp64=False, **kw), pcg_solve, (1e-5,))
run("starmg_fp32", lambda: st.StarMG((n, n, n), w, fp64=False, **kw), mg_solve, (1e-5,))
run("starmg_fp64", lambda: st.StarMG((n, n, n), w, fp64=True, **kw), mg_solve, (1e-5, 1e-10))
run("starcg_fp64", lambda: st.StarCG((n, n, n), w, fp64=True, **kw), cg_solve, (1e-5, 1e-10))
