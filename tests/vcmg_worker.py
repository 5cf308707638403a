"""Worker of the two-rank StarMG tests on the variable-coefficient operator (launched by conftest.run_ranks):
-div(kappa grad) with the smooth coefficient on 32^3 between AntiMirror walls in fp64, every level a realized domain of
the one process group. Every rank compares its part of u after one cycle bitwise with ops.varcoef_mg_cycle_reference
and its parts of every level's kappa with the restricted coefficient, then solves on and prints `history` with
float.hex, which the test requires to be equal across ranks. Host backend: the TCP group; MP_DEVICE=1: the ranks share
GPU 0."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import vcmg_cases as cases
from algebra_cases import same_bits
from stencil2_amd.ops import restrict_reference


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    dtype = torch.float64
    kappa, bc, w, _, _ = cases.problem(cases.CONVERGENCE["smooth_antimirror"], dtype)
    m, f = cases.make_mg(st, backend, cases.SIZE, w, kappa, bc, dtype, group=g, methods=methods)
    m.cycle()
    m.synchronize()
    want = cases.cycle_reference(m, f, kappa, bc)
    bad = 0
    dd = m.domain
    for di in range(dd.num_domains()):
        o, s = dd.domain(di).origin(), dd.domain(di).size()
        bad += int(not same_bits(m.solution(di).cpu(), want[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x].contiguous()))
    k = kappa
    for l in range(m.levels):
        ld = m.level_domain(l)
        for di in range(ld.num_domains()):
            o, s = ld.domain(di).origin(), ld.domain(di).size()
            bad += int(not same_bits(m.level_kappa(l, di).cpu(), k[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x].contiguous()))
        k = restrict_reference(k)
    cycles, rel = m.solve(tol=1e-6)
    bad += int(rel >= 1e-6) + int(cycles > 12)
    print(f"rank {g.rank()} of {g.size()} vcmg bad {bad} levels {m.levels} dim {dd.placement_dim()} cycles {cycles}",
          flush=True)
    print(f"vcmg history {' '.join(h.hex() for h in m.history)}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
