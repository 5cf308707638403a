"""Worker of the two-rank StarPCG tests (launched by conftest.run_ranks): -div(kappa grad) with a contrast of 100 on
16^3 between the mixed walls of pcg_cases, fp64 outside and an fp32 cycle inside, the outer domain and every level of
the preconditioner realized on the one process group. Every rank prints the solver's (iters, relres) with float.hex,
which the test requires to be equal across ranks, and compares the iteration count and its part of the solution with a
one-rank solve of the same decomposition (two sub-domains on its own single group). Host backend: the TCP group;
MP_DEVICE=1: the ranks share GPU 0."""
import faulthandler
import os
import sys

import stencil2_amd as st
import pcg_cases as cases
from algebra_cases import gather_solution
from stencil2_amd.ops import operator_varcoef


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    size, tol = (16, 16, 16), 1e-10
    w, bc = operator_varcoef(0.0), cases.walls("mixed")
    kappa, f = cases.kappa_field(size, 100.0), cases.rhs(size, False)
    m = cases.make_pcg(st, backend, size, w, bc, cases.F64, cases.F32, kappa=kappa, f=f, group=g, methods=methods)
    iters, rel = m.solve(tol=tol)
    one = cases.make_pcg(st, backend, size, w, bc, cases.F64, cases.F32, kappa=kappa, f=f, gpus=(0, 0))
    iters1, rel1 = one.solve(tol=tol)
    want = gather_solution(one)
    bad = int(abs(iters - iters1) > 1) + int(rel >= tol) + int(m.preconditioner.levels != one.preconditioner.levels)
    m.synchronize()
    dd = m.domain
    err = 0.0
    for di in range(dd.num_domains()):
        o, s = dd.domain(di).origin(), dd.domain(di).size()
        part = want[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x]
        err = max(err, float((m.solution(di).cpu() - part).abs().max()) / float(want.abs().max()))
    bad += int(err > 1e-8)
    print(f"rank {g.rank()} of {g.size()} pcg bad {bad} levels {m.preconditioner.levels} (one rank: iters {iters1}, "
          f"relres {rel1:.3e}) dim {dd.placement_dim()} solution err {err:.3e}", flush=True)
    print(cases.hexline(iters, rel), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
