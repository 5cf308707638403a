"""Worker of the two-rank field algebra tests (launched by conftest.run_ranks): DistributedDomain.axpby with stats on
(40, 24, 36) in fp32, and StarCG on (16, 12, 10) in fp64. Exact integer data: every rank compares the collective stats
with the exact values. Random data: every rank prints float.hex of every field, and the solver's (iters, relres); the
test requires the ranks' lines to be equal. Host backend: the TCP group; MP_DEVICE=1: the ranks share GPU 0."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import algebra_cases as cases
import reduce_cases as rc


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    size, dtype = cases.DD_SIZE, torch.float32
    dd, qa, qb, (qc,) = rc.make_domain(st, backend, size, dtype, group=g, methods=methods, extra=(dtype,))
    rc.poison(dd, [qa, qb, qc])
    A, B = rc.exact_field(size, 21), rc.exact_field(size, 22)  # the same seeded fields on every rank
    rc.put(dd, qb, True, A.to(dtype))
    rc.put(dd, qc, False, B.to(dtype))
    s = dd.axpby(qa, 2, qb, -3, qc, y_curr=False, stats=True)
    want = rc.expect_exact(2 * A - 3 * B)
    bad = sum(getattr(s, k) != want[k] for k in rc.FIELDS)
    again = dd.reduce(qa)
    bad += sum(getattr(again, k) != want[k] for k in rc.FIELDS)
    local = dd.axpby(qa, 2, qb, -3, qc, y_curr=False, stats=True, local=True)
    bad += not 0 < local.count < A.numel()
    # the random field: merged in rank order on every rank, so the bits agree
    rc.put(dd, qb, True, rc.random_field(size, dtype, 61))
    rc.put(dd, qc, False, rc.random_field(size, dtype, 62))
    s = dd.axpby(qa, 1.3, qb, 2.9, qc, y_curr=False, stats=True)
    paths = [st.ops.field_axpby_launch_info(dd, di, qa, 1.3, qb, 2.9, qc)["path"] for di in range(dd.num_domains())]
    print(f"rank {g.rank()} of {g.size()} axpby bad {bad} dim {dd.placement_dim()} paths {paths} local {local.count}",
          flush=True)
    print("hex " + cases.hexline(s), flush=True)
    # the solver: every reduction is collective, so every rank stops at the same iteration with the same residual
    m, f = cases.make_cg(st, backend, cases.helmholtz(), cases.walls(0.0), torch.float64, group=g, methods=methods)
    iters, relres = m.solve(tol=cases.CG_TOL[torch.float64], max_iters=1000)
    print(f"cg iters {iters} relres {relres.hex()}", flush=True)
    sys.exit(1 if bad or relres >= cases.CG_TOL[torch.float64] else 0)


if __name__ == "__main__":
    main()
