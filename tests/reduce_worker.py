"""Worker of the two-rank field reduction tests (launched by conftest.run_ranks): DistributedDomain.reduce on
(40, 24, 36) in fp32. Exact integer data: every rank compares the collective result with the exact values. Random data:
every rank prints float.hex of every field, and the test requires the ranks' lines to be equal. Host backend: the TCP
group; MP_DEVICE=1: the ranks share GPU 0."""
import faulthandler
import os
import sys

import torch

import stencil2_amd as st
import reduce_cases as cases


def main():
    faulthandler.enable()
    faulthandler.dump_traceback_later(float(os.environ.get("MP_STALL_DUMP_S", "40")), repeat=True)
    device = os.environ.get("MP_DEVICE") == "1"
    backend = st.Backend.Device if device else st.Backend.Host
    methods = st.MethodFlags.None_
    for name in os.environ.get("MP_METHODS", "All").split("|"):
        methods = methods | getattr(st.MethodFlags, name)
    g = st.init_process_group()
    size = cases.DD_SIZE
    dd, qa, qb, _ = cases.make_domain(st, backend, size, torch.float32, group=g, methods=methods)
    A, B = cases.exact_field(size, 21), cases.exact_field(size, 22)  # the same seeded fields on every rank
    cases.fill_dd(dd, qa, qb, A.float(), B.float())
    bad = 0
    for got, want in ((dd.reduce(qa), cases.expect_exact(A)), (dd.residual(qa), cases.expect_exact(A, B)),
                      (dd.reduce(qa, other=qb, other_curr=True), cases.expect_exact(A, B))):
        bad += sum(getattr(got, k) != want[k] for k in cases.FIELDS)
    bad += dd.dot(qa, qb) != int((A * B).sum()) or dd.norm(qa, 1) != int(A.abs().sum())
    local = dd.reduce(qa, local=True)
    bad += not 0 < local.count < A.numel()
    # the random field: merged in rank order on every rank, so the bits agree
    cases.put(dd, qa, True, cases.random_field(size, torch.float32, 31))
    cases.put(dd, qb, True, cases.random_field(size, torch.float32, 32))
    s = dd.reduce(qa, other=qb, other_curr=True)
    paths = [st.ops.field_reduce_launch_info(dd, di, qa)["path"] for di in range(dd.num_domains())]
    print(f"rank {g.rank()} of {g.size()} reduce bad {bad} dim {dd.placement_dim()} paths {paths} local {local.count}",
          flush=True)
    print("hex " + " ".join(f"{k}={float(getattr(s, k)).hex()}" for k in cases.FIELDS), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
