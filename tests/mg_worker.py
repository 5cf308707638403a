"""Worker of the two-rank StarMG tests (launched by conftest.run_ranks): -Laplacian on 32^3 between AntiMirror walls
in fp64, every level a realized domain of the one process group. Every rank prints the solver's (cycles, relres) with
float.hex, which the test requires to be equal across ranks, and compares its part of the solution with a one-rank
solve of the same decomposition (two sub-domains on its own single group). Host backend: the TCP group; MP_DEVICE=1:
the ranks share GPU 0."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import mg_cases as cases
from algebra_cases import gather_solution


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    dtype, tol = torch.float64, 1e-10
    w, bc = cases.poisson(), cases.all_antimirror()
    m, f = cases.make_mg(st, backend, cases.SIZE, w, bc, dtype, group=g, methods=methods)
    cycles, rel = m.solve(tol=tol)
    one, _ = cases.make_mg(st, backend, cases.SIZE, w, bc, dtype, gpus=(0, 0))
    cycles1, rel1 = one.solve(tol=tol)
    want = gather_solution(one)
    bad = int(cycles != cycles1) + int(m.levels != one.levels) + int(rel >= tol)
    m.synchronize()
    dd = m.domain
    err = 0.0
    for di in range(dd.num_domains()):
        o, s = dd.domain(di).origin(), dd.domain(di).size()
        part = want[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x]
        err = max(err, float((m.solution(di).cpu() - part).abs().max()) / float(want.abs().max()))
    bad += int(err > 1e-9)
    print(f"rank {g.rank()} of {g.size()} mg bad {bad} levels {m.levels} (one rank: {one.levels}, cycles {cycles1}) "
          f"dim {dd.placement_dim()} solution err {err:.3e}", flush=True)
    print(f"mg cycles {cycles} relres {rel.hex()}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
