"""Worker of the two-rank box stencil tests (launched by conftest.run_ranks): BoxStencil3D in fp32 on (40, 24, 36),
4 steps; every rank compares its interior with its slice of the torch oracle. Host backend: staged over the TCP group;
MP_DEVICE=1: the ranks share GPU 0 (Colocated)."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import box_cases as cases

SIZE, STEPS = (40, 24, 36), 4


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    w = cases.random_box()
    m = st.BoxStencil3D(SIZE, w, gpus=[0], backend=backend, methods=methods, group=g)
    u = cases.global_field(SIZE, torch.float32)  # the same seeded field on every rank
    m.init(lambda gz, gy, gx: u.to(gz.device)[gz % SIZE[2], gy % SIZE[1], gx % SIZE[0]])
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
    paths = [st.ops.box_launch_info(dd, di, 0, w)["path"] for di in range(dd.num_domains())]
    print(f"rank {g.rank()} of {g.size()} box bad {bad} dim {dd.placement_dim()} paths {paths} "
          f"plan {sorted({str(e.method) for e in dd.plan()})}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
