"""Worker of the two-rank variable-coefficient stencil tests (launched by conftest.run_ranks): VarCoefStencil3D in fp32
on (40, 24, 36), 3 steps; every rank compares its interior with its slice of the torch oracle. Host backend: staged over
the TCP group; MP_DEVICE=1: the ranks share GPU 0 (Colocated)."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import varcoef_cases as cases

SIZE, STEPS = (40, 24, 36), 3


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    w = cases.random_weights()
    # the same seeded fields on every rank
    m = cases.make_model(st, backend, SIZE, torch.float32, [0], w=w, group=g, methods=methods)
    m.run(STEPS)
    m.synchronize()
    want = cases.oracle(SIZE, torch.float32, STEPS)
    bad = 0
    dd = m.domain
    for di in range(dd.num_domains()):
        d = dd.domain(di)
        o, s = d.origin(), d.size()
        got = m.interior(di).cpu()
        bad += int((got != want[o.z:o.z + s.z, o.y:o.y + s.y, o.x:o.x + s.x]).sum())
    paths = [st.ops.varcoef_launch_info(dd, di, m.u, m.kappa, w)["path"] for di in range(dd.num_domains())]
    print(f"rank {g.rank()} of {g.size()} varcoef bad {bad} dim {dd.placement_dim()} paths {paths} "
          f"plan {sorted({str(e.method) for e in dd.plan()})}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
