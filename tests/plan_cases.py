"""Cases shared by test_plan_pinned.py (host backend) and test_gpu_plan_pinned.py (device backend, device 0 only):
DistributedDomain.plan_summary() after realize(), compared byte for byte with the text fixtures under
tests/golden/plans/ (one per single-process case, one per rank of a multi-rank case). The summary lists every
sub-domain (device, index, size, origin), every planned message per transport (ranks, devices, direction, bytes) and
the bytes per transport summed over all ranks, so a change of placement, of the transport ladder or of the packed
sizes shows as a changed text.

The fixtures are recorded by this module, from the repository root:

    python tests/plan_cases.py            # the host-backend fixtures
    python tests/plan_cases.py --gpu      # the device-backend fixtures (needs the GPU)

Every case is recorded twice; a case whose two recordings differ is reported and not written."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plans")
WORKER = os.path.join(HERE, "mp_worker.py")
BEGIN, END = "@@plan {}@@", "@@end plan@@"

# ---- single process: name -> (size, gpus, methods, radius, boundary) ----
P, YZ = "periodic", "open-x"
SINGLE = {
    "one-all-r1": ((13, 11, 9), [0], "All", "r1", P),
    "one-staged-fec": ((13, 11, 9), [0], "Staged", "fec", P),
    "one-all-asym-openx": ((16, 12, 10), [0], "All", "asym", YZ),
    "two-all-r1": ((13, 11, 9), [0, 0], "All", "r1", P),
    "two-all-fec": ((16, 12, 10), [0, 0], "All", "fec", P),
    "two-staged-r1": ((16, 12, 10), [0, 0], "Staged", "r1", P),
    "two-staged-asym": ((13, 11, 9), [0, 0], "Staged", "asym", P),
    "two-all-fec-openx": ((13, 11, 9), [0, 0], "All", "fec", YZ),
    "four-all-r1": ((16, 12, 10), [0, 0, 0, 0], "All", "r1", P),
    "four-all-fec": ((13, 11, 9), [0, 0, 0, 0], "All", "fec", P),
    "four-staged-fec": ((16, 12, 10), [0, 0, 0, 0], "Staged", "fec", P),
    "four-staged-asym-openx": ((16, 12, 10), [0, 0, 0, 0], "Staged", "asym", YZ),
    "four-all-asym": ((13, 11, 9), [0, 0, 0, 0], "All", "asym", P),
}
# ---- ranks of one TCP group, host backend, 16x12x10 with faces 2, edges 1, corners 1: name -> (ranks, two nodes) ----
RANKS = {"ranks2": (2, False), "ranks3": (3, False), "ranks4": (4, False), "ranks4-two-nodes": (4, True)}
RANKS_SIZE, RANKS_RADIUS = (16, 12, 10), "fec"

# ---- device backend, every sub-domain on device 0, 16x12x10: name -> (gpus, methods, peer copy) ----
GPU_SIZE, GPU_RADIUS = (16, 12, 10), "fec"
GPU_SINGLE = {
    "gpu-two-all": ([0, 0], "All", "Store"),            # plans Kernel
    "gpu-two-peercopy-engine": ([0, 0], "PeerCopy", "Engine"),
    "gpu-two-rccl": ([0, 0], "Rccl", "Store"),
    "gpu-two-staged": ([0, 0], "Staged", "Store"),
    "gpu-three-all": ([0, 0, 0], "All", "Store"),
}
# two ranks sharing the GPU: name -> extra environment of the ranks
GPU_RANKS = {"gpu-ranks2-all": {}, "gpu-ranks2-all-ipc-probe-fail": {"MP_IPC_PROBE_FAIL": "1"}}


def radii(st):
    a = st.Radius.constant(0)  # +x2-x1
    a.set_dir(1, 0, 0, 2)
    a.set_dir(-1, 0, 0, 1)
    return {"r1": st.Radius.constant(1), "fec": st.Radius.face_edge_corner(2, 1, 1), "asym": a}


def realize(st, backend, size, gpus, methods, radius, boundary=P, peer_copy="Store", group=None):
    dd = st.DistributedDomain(*size, group=group if group is not None else st.make_single_group())
    dd.set_backend(backend)
    tr = st.TransportOptions()
    tr.peer_copy = getattr(st.TransportOptions.Copy, peer_copy)
    dd.set_transport_options(tr)
    dd.set_radius(radii(st)[radius])
    if boundary == YZ:
        dd.set_boundary(st.Boundary.axes(False, True, True))
    dd.set_gpus(list(gpus))
    dd.set_methods(getattr(st.MethodFlags, methods))
    dd.set_plan_file("")
    q = dd.add_data("c", torch.int64)
    dd.realize()
    return dd, q


def single_summary(st, name):
    size, gpus, methods, radius, boundary = SINGLE[name]
    return realize(st, st.Backend.Host, size, gpus, methods, radius, boundary)[0].plan_summary()


def gpu_single_summary(st, name):
    """the summary of a working plan: one exchange against the coordinate oracle first"""
    from stencil2_amd.utils.testing import check_exchange, fill_coords
    gpus, methods, peer_copy = GPU_SINGLE[name]
    dd, q = realize(st, st.Backend.Device, GPU_SIZE, gpus, methods, GPU_RADIUS, peer_copy=peer_copy)
    fill_coords(dd, q)
    dd.exchange()
    assert check_exchange(dd, q, radii(st)[GPU_RADIUS]) == 0
    return dd.plan_summary()


def rank_summaries(n, size, radius, env_extra=None, per_rank_env=None):
    """the `plan` scenario of mp_worker.py on n ranks: one exchange against the coordinate oracle, then every rank's
    summary between markers"""
    from conftest import run_ranks
    outs = run_ranks(n, WORKER, ["plan", radius, ",".join(map(str, size))], env_extra=env_extra,
                     per_rank_env=per_rank_env, timeout=120)
    texts = []
    for r, (rc, out) in enumerate(outs):
        assert rc == 0 and f"rank {r} plan bad 0" in out, out[-3000:]
        texts.append(out.split(BEGIN.format(r), 1)[1].split(END, 1)[0])
    return texts


def host_rank_summaries(name):
    n, two_nodes = RANKS[name]
    per_rank = (lambda r: {"STENCIL_HOSTNAME": f"node{r // 2}"}) if two_nodes else None
    return rank_summaries(n, RANKS_SIZE, RANKS_RADIUS, per_rank_env=per_rank)


def gpu_rank_summaries(name):
    env = {"MP_DEVICE": "1", "MP_METHODS": "All", "STENCIL_WAIT_TIMEOUT": "20", **GPU_RANKS[name]}
    return rank_summaries(2, GPU_SIZE, GPU_RADIUS, env_extra=env)


def fixture(name, rank=None):
    path = os.path.join(GOLDEN, name + ("" if rank is None else f"-rank{rank}") + ".txt")
    with open(path, newline="") as f:
        return f.read()


def check_single(name, text):
    assert text == fixture(name), f"plan of {name} differs from tests/golden/plans/{name}.txt:\n{text}"


def check_ranks(name, texts):
    for r, text in enumerate(texts):
        assert text == fixture(name, r), f"plan of {name}, rank {r}, differs from its fixture:\n{text}"


# ---- recording ----
def record(gpu):
    import stencil2_amd as st
    if gpu:
        takes = [(n, lambda n=n: [gpu_single_summary(st, n)], False) for n in GPU_SINGLE]
        takes += [(n, lambda n=n: gpu_rank_summaries(n), True) for n in GPU_RANKS]
    else:
        takes = [(n, lambda n=n: [single_summary(st, n)], False) for n in SINGLE]
        takes += [(n, lambda n=n: host_rank_summaries(n), True) for n in RANKS]
    os.makedirs(GOLDEN, exist_ok=True)
    dropped = []
    for name, take, ranked in takes:
        first, second = take(), take()
        if first != second:
            dropped.append(name)
            continue
        for r, text in enumerate(first):
            path = os.path.join(GOLDEN, name + (f"-rank{r}" if ranked else "") + ".txt")
            with open(path, "w", newline="") as f:
                f.write(text)
            print(f"recorded {os.path.relpath(path, HERE)} ({len(text)} B)")
    print("dropped (two recordings differ):", dropped or "none")
    return 1 if dropped else 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.exit(record("--gpu" in sys.argv))
