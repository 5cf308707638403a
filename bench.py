#!/usr/bin/env python3
"""Headline benchmark: Jacobi3D weak scaling, 512^3 cells per GPU, fp32, one process per GPU.

Metric (BASELINE.json): "halo-exchange GB/s + Jacobi3D Gcells/s, 512^3/GPU weak scaling at 1/2/4/8 MI355X".
`value` is the whole-job Jacobi3D throughput in Gcells/s (global cells x steps / time). One step is the
reference's full iteration (bin/jacobi3d.cu:265-346): interior stencil overlapped with the halo exchange of all
faces (periodic), exterior stencil, swap. Every GPU holds exactly 512^3 cells (--grid exact); the decomposition is
the NodeAware partitioner's MaxLink choice for the xGMI mesh (1x1xN slabs: two faces per GPU, each on its own
link); --grid cbrt runs the reference's cube rule (512 * N^0.33333 per axis: 645/813/1024 for N=2/4/8) and
--partition interface the reference's cut rule.
A plain run does what the headline needs and nothing else: set up, warm up (with the fused-triple schedule choice),
time exactly --steps steps, write --dump-outputs, print the JSON line. --full adds the secondary sections to the same
line: the halo-exchange GB/s of an exchange-only loop on the same decomposition (bin/bench_exchange.cu definition:
aggregate halo bytes / time), the same steps with every halo copied (extra.with_exchange) and the per-transport sweep.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
  N>1 runs one rank per GPU. Under torch.distributed.run (WORLD_SIZE set) it must equal WORLD_SIZE; without a
  launcher, bench.py itself spawns N fresh child ranks (stencil2_amd/launch.py, loaded by path) before importing
  torch or touching the GPU, waits for them with a bounded timeout, stops every sibling when one fails and exits with
  the failing rank's code. Rank 0 prints the JSON line (reference: one rank per GPU from the job script,
  scripts/summit/weak_256n.sh:26-30).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time


def weak_grid(st, per_gpu: int, n: int, rule: str, axis_cost, objective) -> tuple:
    """Global grid of the weak-scaling run on n GPUs.

    cbrt: the reference's cube of side per_gpu * n^(1/3) (bin/jacobi3d.cu:167-169).
    exact: every sub-domain exactly per_gpu^3, so per-GPU work is the N=1 work to the cell; the decomposition d is
    the partitioner's choice for n cubes (MaxLink on the node's xGMI mesh: 1x1xN slabs, two faces per GPU on two
    links; Interface: the reference's greedy cut of the cbrt-scaled cube, 1x1x2 / 1x2x2 / 1x2x4), the grid is
    per_gpu x d.
    """
    L = st.models.weak_scaled_size(per_gpu, n)
    if rule == "cbrt" or n == 1:
        return (L, L, L)
    r = st.Radius.constant(0)
    r.set_face(1)
    cost = st.Dim3(*axis_cost)
    if objective == st.PartitionObjective.MaxLink:
        # every factorization d of n, scored on the grid of n per_gpu^3 cubes it forms (busiest link, total)
        best = None
        for dx in range(1, n + 1):
            for dy in range(1, n // dx + 1):
                if n % (dx * dy):
                    continue
                dz = n // (dx * dy)
                g = st.Dim3(per_gpu * dx, per_gpu * dy, per_gpu * dz)
                c = st.NodePartition.link_cost(g, st.Dim3(dx, dy, dz), r, cost)
                key = (c, dx, dy)
                if best is None or key < best[0]:
                    best = (key, st.Dim3(dx, dy, dz))
        d = best[1]
    else:
        d = st.NodePartition(st.Dim3(L, L, L), r, 1, n, cost).dim()
    grid = (per_gpu * d.x, per_gpu * d.y, per_gpu * d.z)
    p = st.NodePartition(st.Dim3(*grid), r, 1, n, cost, objective)
    if p.dim() != d or any(p.subdomain_size(st.Dim3(i, j, k)) != st.Dim3(per_gpu, per_gpu, per_gpu)
                           for i in range(d.x) for j in range(d.y) for k in range(d.z)):
        return (L, L, L)  # the partitioner would not cut the scaled grid into equal cubes: the reference rule
    return grid


class Env:
    """What the bench needs from the device side, with a host-backend stand-in (--cpu: the CPU path of BASELINE.json
    config 1, and the CPU tests of this script's control flow)."""

    def __init__(self, torch, dist, cpu: bool, world: int, red_dev: str):
        self.torch, self.dist, self.cpu, self.world, self.red_dev = torch, dist, cpu, world, red_dev

    def sync(self):
        if not self.cpu:
            self.torch.cuda.synchronize()

    def barrier(self):
        self.sync()
        if self.world > 1:
            self.dist.barrier()
        self.sync()

    def agreed_max(self, v: float) -> float:
        t = self.torch.tensor([float(v)], dtype=self.torch.float64, device=self.red_dev)
        if self.world > 1:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def stream(self):
        return None if self.cpu else self.torch.cuda.Stream()


def time_exchanges(env, dd, iters: int, xbytes: int, log: bool = False) -> dict:
    """Blocking exchange()+swap() (bin/bench_exchange.cu:39-63) and the same exchanges stream-ordered on one stream,
    max over ranks; GB/s = aggregate halo bytes over all ranks / time (the reference's definition). log: device
    timestamps of the fused co-located kernels (wait vs copy) over the blocking loop."""
    for _ in range(3):  # untimed: the first full exchanges after wrapped pairs touch cold halo lines
        dd.exchange()
        dd.swap()
    if log:
        dd.set_transport_log(iters)
    env.barrier()
    t = time.perf_counter()
    for _ in range(iters):
        dd.exchange()
        dd.swap()
    env.sync()
    el = env.agreed_max(time.perf_counter() - t)
    rec = {"iters": iters, "halo_bytes": int(xbytes), "exchange_ms": round(el / iters * 1e3, 4),
           "GBps": round(xbytes * iters / el / 1e9, 3)}
    if log:
        rec["colo_kernels_us"] = colo_breakdown(dd.transport_log(0))
        dd.set_transport_log(0)
    xs = env.stream()
    if xs is not None:
        for _ in range(3):  # untimed: the first launches on a new stream create its hardware queue (~ms)
            dd.exchange_async(xs.cuda_stream, 0)
            dd.swap()
        xs.synchronize()
        dd.sync_exchange()
        env.barrier()
        t = time.perf_counter()
        for _ in range(iters):
            dd.exchange_async(xs.cuda_stream, 0)
            dd.swap()
        xs.synchronize()
        dd.sync_exchange()
        el2 = env.agreed_max(time.perf_counter() - t)
        rec["stream_GBps"] = round(xbytes * iters / el2 / 1e9, 3)
    return rec


def used_methods(st, dd) -> str:
    """The transports that carry halo bytes in this realized domain (methods() is the enabled set)."""
    M = st.MethodFlags
    used = M.None_
    for f in (M.Kernel, M.PeerCopy, M.Colocated, M.Rccl, M.Staged):
        if dd.exchange_bytes_for_method(f) > 0:
            used = used | f
    return st.methods_to_string(used)


def probe_iters(env, dd, cap: int) -> int:
    """Timed exchanges of a sweep entry: as many as fit in ~1 s (agreed over ranks), at most cap."""
    for _ in range(2):
        dd.exchange()
        dd.swap()
    env.sync()
    t = time.perf_counter()
    dd.exchange()
    dd.swap()
    probe = env.agreed_max(time.perf_counter() - t)
    return int(max(1, min(cap, 1.0 / max(probe, 1e-6))))


def transport_sweep(st, env, args, world, rank, device, ndev, axis_cost, objective, topt_base, methods_base) -> dict:
    """Exchange-only GB/s of the headline decomposition with each transport set in turn, then the entries no
    per-rank transport covers, so one multi-GPU run yields the whole ladder (reference: src/stencil.cu:163-194
    method ladder; scripts/summit/weak_256n.sh:26-30 per-method sweeps):

      colo_store / colo_engine / colo_ipcevent / rccl / staged   the headline decomposition, one transport set each
                                                                 (rccl at N = 1: the RCCL loopback, methods Rccl only)
      ref_rule     the cbrt cube cut by the reference's greedy Interface rule (2x2x2 at N = 8: the
                   bench_exchange --x 1024 --y 1024 --z 1024 --fr 2 config)
      astaroth_q8  BASELINE config 4's exchange: 8 fp32 quantities, radius 3 in all 26 directions, on the
                   reference-rule cube, with the headline's transports (bin/astaroth_sim.cu:184-195)
      peer_store / peer_engine   the reference's default single-process multi-GPU run: rank 0 alone realizes the
                   headline decomposition over devices 0..N-1 (include/stencil/stencil.hpp:192-198) with
                   PeerCopy|Kernel -- direct xGMI stores into the peer's halo, then pack + hipMemcpyPeerAsync +
                   unpack (include/stencil/tx_cuda.cuh:106-170); the other ranks wait at a barrier. On a box with
                   fewer GPUs than ranks the devices repeat, and `devices_used` says how many were really used.

    Radius-2 faces, one fp32 quantity (the depth-2 exchange of a fused pair) unless stated. Each entry realizes its
    own domain on a fresh native process group with a short timeout, so a transport that fails on one rank costs that
    entry (an "error" string), not the run; an RCCL communicator that cannot be created is bounded by the same timeout
    (non-blocking creation + abort) and reported as `rccl_status`. The section stops starting entries after
    --sweep-budget seconds (agreed over ranks)."""
    M = st.MethodFlags
    C = st.TransportOptions.Completion
    rccl_set = M.Rccl if world == 1 else M.Rccl | M.Kernel
    sets = [("colo_store", M.Colocated | M.Kernel, {"copy": "store", "completion": C.Kernel}),
            ("colo_engine", M.Colocated | M.Kernel, {"copy": "engine", "completion": C.Kernel}),
            ("colo_ipcevent", M.Colocated | M.Kernel, {"copy": "store", "completion": C.IpcEvent}),
            ("rccl", rccl_set, {}), ("staged", M.Staged | M.Kernel, {}),
            ("ref_rule", M.All, {"grid": "ref"}),
            ("astaroth_q8", methods_base, {"grid": "ref", "q": 8, "radius": 3}),
            ("peer_store", M.PeerCopy | M.Kernel, {"peer": "store"}),
            ("peer_engine", M.PeerCopy | M.Kernel, {"peer": "engine"})]
    if args.cpu:  # host backend: only Staged and same-rank copies exist
        sets = [s for s in sets if s[0] in ("staged", "ref_rule", "astaroth_q8", "peer_store")]
    out = {}
    t_start = time.perf_counter()
    stall = os.environ.get("STENCIL_RCCL_STALL_RANK")
    if os.environ.get("STENCIL_BENCH_SWEEP_HANG"):  # test hook: a sweep entry that never returns (arm_deadline)
        time.sleep(1e6)
    for name, m, o in sets:
        if env.agreed_max(time.perf_counter() - t_start) > args.sweep_budget:
            out[name] = {"skipped": f"sweep budget {args.sweep_budget:.0f} s spent"}
            continue
        rec = {}
        ok = 1.0
        dd = None
        peer = "peer" in o
        if rank == 0:
            print(f"[bench] transport {name}: starting", file=sys.stderr, flush=True)
        try:
            if o.get("grid") == "ref":
                L = st.models.weak_scaled_size(args.per_gpu, world)
                g, obj, cost = (L, L, L), st.PartitionObjective.Interface, (1, 1, 1)
            else:
                g, obj, cost = weak_grid(st, args.per_gpu, world, args.grid, axis_cost, objective), objective, axis_cost
            if peer and rank != 0:
                rec["by"] = "rank 0"
            else:
                grp = st.make_single_group() if peer else st.init_process_group(set_default=False, timeout_s=15.0)
                dd = st.DistributedDomain(*g, group=grp)
                if args.cpu:
                    dd.set_backend(st.Backend.Host)
                r = st.Radius.constant(o.get("radius", 0))
                if "radius" not in o:
                    r.set_face(2)
                dd.set_radius(r)
                for q in range(o.get("q", 1)):
                    dd.add_data(f"q{q}", env.torch.float32)
                dd.set_methods(m)
                gpus = [k % max(1, ndev) for k in range(world)] if peer else [device]
                dd.set_gpus(gpus)
                dd.set_axis_cost(st.Dim3(*cost))
                dd.set_partition_objective(obj)
                dd.set_plan_file("")
                dd.set_interior_align(args.interior_align)
                dd.set_shared_halo_line(args.shared_halo_line == 1)
                topt = st.TransportOptions()
                topt.inbox = topt_base.inbox
                topt.completion = o.get("completion", topt_base.completion)
                topt.fuse_flags = topt_base.fuse_flags
                cp = o.get("copy")
                topt.colo_copy = topt_base.colo_copy if cp is None else (
                    topt.Copy.Engine if cp == "engine" else topt.Copy.Store)
                topt.peer_copy = topt.Copy.Engine if o.get("peer") == "engine" else topt.Copy.Store
                topt.wait_timeout = 10.0  # a failing entry gives up within seconds, not minutes
                if stall is not None:  # rehearses a rank stuck before RCCL communicator creation
                    topt.stall_rccl_init_rank = int(stall)
                dd.set_transport_options(topt)
                dd.realize()
                pd = dd.placement_dim()
                rec["grid"] = list(g)
                rec["decomposition"] = f"{pd.x}x{pd.y}x{pd.z}"
                rec["asked"] = st.methods_to_string(m)
                rec["realized"] = used_methods(st, dd)
                if dd.rccl_status():
                    rec["rccl_status"] = dd.rccl_status()
                    if dd.rccl_status() != "ok":
                        rec["error"] = f"RCCL communicator: {dd.rccl_status()} (halos ran host-staged)"
                if peer:
                    rec["devices_used"] = len(set(gpus))
                    rec["device_count"] = ndev
                rec["bytes_by_method"] = {st.methods_to_string(f): int(dd.exchange_bytes_for_method(f))
                                          for f in (M.Kernel, M.PeerCopy, M.Colocated, M.Rccl, M.Staged)
                                          if dd.exchange_bytes_for_method(f) > 0}
                penv = Env(env.torch, env.dist, env.cpu, 1, env.red_dev) if peer else env
                iters = probe_iters(penv, dd, args.exchange_iters)
                colo = dd.exchange_bytes_for_method(M.Colocated) > 0 and topt.completion != C.StreamOp
                rec.update(time_exchanges(penv, dd, iters, int(dd.exchange_bytes_for_method(M.All)),
                                          log=colo and not args.cpu))
        except Exception as e:  # noqa: BLE001 -- one transport failing must not end the run
            ok = 0.0
            rec["error"] = f"{type(e).__name__}: {str(e)[:300]}"
        del dd
        if peer:
            env.barrier()  # the other ranks wait here while rank 0 drives every GPU
        if env.agreed_max(1.0 - ok) > 0 and "error" not in rec:
            rec["error"] = "failed on another rank"
        out[name] = rec
        if rank == 0:
            print(f"[bench] transport {name}: {rec}", file=sys.stderr, flush=True)
    return out


def colo_breakdown(log) -> dict:
    """Median phases (us) of the fused co-located transport kernels from DistributedDomain.transport_log: per
    exchange {send start, after the credit wait, after the copies, signal, recv start, after the arrival wait, after
    the copies, signal} in 100-MHz ticks (0: that kernel did not run / that phase does not exist)."""
    import statistics

    def med(vals):
        vals = [v for v in vals if v is not None and v >= 0]
        return round(statistics.median(vals) / 100.0, 2) if vals else None

    def ph(e, a, b):
        return e[b] - e[a] if e[a] and e[b] else None

    return {"send_wait": med([ph(e, 0, 1) for e in log]), "send_copy": med([ph(e, 1, 2) for e in log]),
            "send_signal": med([ph(e, 2, 3) for e in log]), "recv_wait": med([ph(e, 4, 5) for e in log]),
            "recv_copy": med([ph(e, 5, 6) for e in log]), "recv_signal": med([ph(e, 6, 7) for e in log]),
            "send_end_to_recv_start": med([ph(e, 3, 4) for e in log]), "exchanges": len(log)}


def _gpus_sysfs() -> int:
    """GPUs of this node from the KFD topology (no HIP call: the HIP runtime must not start before the queue limit
    below is set)."""
    import glob
    n = 0
    for f in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/gpu_id"):
        try:
            n += int(open(f).read().strip() or 0) != 0
        except (OSError, ValueError):
            pass
    return n


def _limit_queues_when_sharing():
    """Ranks sharing one GPU (a rehearsal of the multi-GPU run on a smaller box): keep ranks x hardware queues per
    process <= 8. Beyond that the GPU time-slices the processes' queues and every cross-process hand-off waits a
    scheduling quantum: one MI355X, 8 ranks x 128^3, 39.3 / 6.0 / 2.0 ms per step with 4 / 2 / 1 queues per
    process, 4 ranks 12.4 vs 0.30 ms with 4 vs 2 (profiles/r3/cliff/). One process per GPU is left alone."""
    local = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    ngpu = _gpus_sysfs()
    if ngpu and local > ngpu and "GPU_MAX_HW_QUEUES" not in os.environ:
        per_gpu = -(-local // ngpu)
        os.environ["GPU_MAX_HW_QUEUES"] = str(max(1, 8 // per_gpu))


def _launcher():
    """stencil2_amd/launch.py without importing the package (its __init__ imports torch and the HIP runtime)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stencil2_amd", "launch.py")
    spec = importlib.util.spec_from_file_location("_stencil2_launch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rank_setup(gpus: int, launch_timeout: float, argv: list[str]):
    """None: this process is a rank (run the bench). An int: the exit code of this process (a spawning parent, or a
    --gpus / WORLD_SIZE mismatch). Runs before torch is imported: no HIP call may precede the fork."""
    world = os.environ.get("WORLD_SIZE")
    if world is None:
        if gpus <= 1:
            return None
        return _launcher().spawn_ranks([sys.executable, os.path.abspath(__file__), *argv], gpus,
                                       timeout=launch_timeout if launch_timeout > 0 else None)
    if int(world) != gpus:
        print(f"bench.py: --gpus {gpus} but WORLD_SIZE={world}: the launcher and the bench disagree on the number "
              f"of GPUs; refusing to time a different job than the one asked for", file=sys.stderr, flush=True)
        return 2
    if os.environ.get("STENCIL_BENCH_DRY"):  # launcher tests (CPU): report the rank layout, touch nothing else
        rank = int(os.environ.get("RANK", "0"))
        if os.environ.get("STENCIL_BENCH_DRY_FAIL_RANK") == str(rank):
            return 3
        if os.environ.get("STENCIL_BENCH_DRY_SLEEP"):
            time.sleep(float(os.environ["STENCIL_BENCH_DRY_SLEEP"]))
        print(json.dumps({"rank": rank, "world": int(world), "local_rank": int(os.environ.get("LOCAL_RANK", "-1")),
                          "master": f"{os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')}",
                          "torch_loaded": "torch" in sys.modules}), flush=True)
        return 0
    return None


def build_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-gpu", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="after the headline loop also run the secondary sections: the exchange-only loops (extra.halo_"
                         "exchange_*), the steps with every halo copied (--with-exchange) and the per-transport sweep "
                         "(--transport-sweep). Without it they are skipped and their entries are null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed loop write every rank's field as the timed steps left it (the interior a "
                         "caller of run() reads) to DIR/u_rank<r>.npy, float32; at most 48 MB over all ranks: a larger "
                         "field is sampled at fixed seeded cells (dump_outputs)")
    ap.add_argument("--cpu", action="store_true",
                    help="host backend, no GPU (BASELINE config 1's CPU path; the CPU tests of this script)")
    ap.add_argument("--exchange-iters", type=int, default=20)
    ap.add_argument("--methods", default="all")
    ap.add_argument("--temporal", type=int, default=3,
                    help="steps fused per sweep: 3 = fused triples S(S(S(u))) (one depth-3 exchange per three steps, x "
                         "wrapped in-kernel or read from halos; elsewhere pairs), 2 = fused pairs (one depth-2 exchange "
                         "per two steps), 1 = one exchange + sweep per step; all bitwise equal to single steps")
    ap.add_argument("--wrap", type=int, default=1,
                    help="the sweeps read the periodic image along axes the decomposition leaves whole (no self-copy "
                         "of those halos); 0 = copy every halo")
    ap.add_argument("--with-exchange", choices=["auto", "on", "off"], default="auto",
                    help="--full: after the headline, time the same steps with every halo copied (BASELINE config 2 as "
                         "defined: intra-GPU pack/unpack + compute, the reference's exchange() every iteration) -> "
                         "extra.gcells_with_exchange (auto: on unless --wrap 0 already copies every halo)")
    ap.add_argument("--shared-halo-line", type=int, default=-1,
                    help="row r's +x and row r+1's -x halo share one 128-B line, written once per row by the x-face "
                         "self copies (LocalDomain::set_shared_halo_line). -1 (auto): on for the with-exchange model, "
                         "whose sweeps read the x-halo lines (967 -> 1027 Gcells/s, profiles/r5/f), off for the headline")
    ap.add_argument("--interior-align", type=int, default=128, choices=[64, 128],
                    help="byte alignment of every row's first interior cell: 128 = whole L2 lines per 512-cell row "
                         "(1150-1194 -> 1285-1287 Gcells/s on one MI355X, profiles/r4/i/), 64 = one sector (r1-r3)")
    ap.add_argument("--axis-cost", default="4,3,2",
                    help="NodeAware partition cost per interface cell of x,y,z cuts (1,1,1 = the reference's rule)")
    ap.add_argument("--partition", choices=["maxlink", "interface"], default="maxlink",
                    help="NodeAware cut rule inside the node: maxlink = fewest halo cells on the busiest xGMI link "
                         "(then fewest in total): 1x1xN slabs of 512^3; interface = the reference's greedy minimum "
                         "interface (1x2x2 / 1x2x4)")
    ap.add_argument("--grid", choices=["exact", "cbrt"], default="exact",
                    help="weak-scaling grid: exact = every GPU holds exactly per_gpu^3 cells (global grid = per_gpu x the "
                         "decomposition of the cbrt-scaled cube); cbrt = the reference's rule, a per_gpu*N^(1/3) cube "
                         "(bin/jacobi3d.cu:167-169: 645^3 / 813^3 / 1024^3 at N = 2 / 4 / 8, ragged sub-domains)")
    ap.add_argument("--overlap", choices=["auto", "on", "off"], default="auto",
                    help="interior/exchange/exterior overlap (auto: only when some halo leaves the GPU, and then "
                         "overlapped, pipelined or whole-region sweeps, whichever runs fastest in the warm-up)")
    ap.add_argument("--x2reserve", type=int, default=8,
                    help="overlapped / pipelined sweeps: CUs left to the transport kernels (the warm-up also tries "
                         "half and double)")
    ap.add_argument("--transport", choices=["auto", "fixed"], default="auto",
                    help="N > 1: auto = the warm-up times whole steps (max over ranks) with Colocated over uncached / "
                         "fine-grained / coarse-grained inboxes and with Rccl, and keeps the fastest for the timed loop "
                         "(config.transport_tuned); fixed = --methods / --inbox as given")
    ap.add_argument("--colo-copy", choices=["auto", "store", "engine"], default="store",
                    help="co-located (HIP IPC) halos: the pack kernel stores into the peer's inbox (store, default), or "
                         "a DMA engine copies the packed message (engine); auto: both tried in the warm-up. Engine "
                         "copies never won on one MI355X (profiles/r3/check4, r4/engine), so they are opt-in")
    ap.add_argument("--inbox", choices=["uncached", "fine", "coarse"], default="uncached",
                    help="memory of the co-located receive slots (TransportOptions.inbox)")
    ap.add_argument("--completion", choices=["kernel", "streamop", "ipcevent"], default="kernel",
                    help="co-located arrival/credit signalling: bounded spin kernels, hipStreamWait/WriteValue64, or "
                         "interprocess events with host notify/ack (the reference's design)")
    ap.add_argument("--fuse-flags", type=int, default=1,
                    help="co-located flag waits/signals folded into the pack/unpack kernels (0: separate kernels)")
    ap.add_argument("--self-test", type=int, default=1,
                    help="multi-process: verify the transports on a probe domain first and fall back along "
                         "Colocated -> Rccl -> Staged until every halo arrives correctly")
    ap.add_argument("--tune-steps", type=int, default=8,
                    help="steps per timed round of the transport / overlap choice (N > 1; 0 = no choice)")
    ap.add_argument("--schedule-rounds", type=int, default=3,
                    help="interleaved timing rounds of the fused-triple schedule candidates (sphere weight, leftover "
                         "plan) before the timed loop; 0 = the StencilTune defaults")
    ap.add_argument("--tune-budget", type=float, default=150.0,
                    help="seconds of warm-up tuning (transport + overlap choice, agreed over ranks): once spent, the "
                         "remaining candidates are skipped and the fastest timed so far is kept (config.phases_s)")
    ap.add_argument("--transport-sweep", choices=["auto", "on", "off"], default="auto",
                    help="--full, after the headline: exchange-only GB/s of every transport set on the same "
                         "decomposition, the reference-rule cube, config 4's 8-quantity radius-3 exchange and the "
                         "single-process PeerCopy run (auto: only with N > 1)")
    ap.add_argument("--sweep-budget", type=float, default=60.0,
                    help="seconds after which the transport sweep starts no further entry")
    ap.add_argument("--sweep-deadline", type=float, default=240.0,
                    help="seconds after which a still-running sweep is abandoned: every rank exits 0 behind the "
                         "headline line it already printed (a transport hanging on real links cannot take it)")
    ap.add_argument("--launch-timeout", type=float, default=3000,
                    help="--gpus N>1 without a launcher: seconds before the spawned ranks are stopped (0 = none)")
    ap.add_argument("--tune", default="",
                    help="lab switch: StencilTune fields as name=value[,name=value] (e.g. x3sphw=0.4,nontemporal=0); "
                         "the defaults are the measured best (StencilTune in csrc/include/stencil/kernels/stencil_ops.hpp)")
    return ap.parse_args(argv)


def make_tune(st, args):
    """StencilTune defaults (the measured best) plus --tune overrides; the effective values go into config.tune."""
    tune = st.StencilTune()
    for kv in filter(None, args.tune.split(",")):
        k, v = kv.split("=", 1)
        cur = getattr(tune, k)  # AttributeError names an unknown field
        setattr(tune, k, type(cur)(float(v)) if not isinstance(cur, bool) else bool(int(v)))
    return tune


def tune_record(tune) -> dict:
    return {k: getattr(tune, k) for k in ("x3sched", "x3parts", "x3sphw", "x3left", "x2sphw", "x2early", "x2row",
                                          "nontemporal", "alternate_z", "xcd_remap", "variant")}


def make_transport(st, args, inbox=None):
    topt = st.TransportOptions()
    topt.inbox = {"uncached": topt.Inbox.Uncached, "fine": topt.Inbox.Fine,
                  "coarse": topt.Inbox.Coarse}[inbox or args.inbox]
    topt.colo_copy = topt.Copy.Engine if args.colo_copy == "engine" else topt.Copy.Store
    topt.completion = {"kernel": topt.Completion.Kernel, "streamop": topt.Completion.StreamOp,
                       "ipcevent": topt.Completion.IpcEvent}[args.completion]
    topt.fuse_flags = bool(args.fuse_flags)
    if os.environ.get("STENCIL_PREFLIGHT_FORCE_FAIL"):  # rehearses the fallback (scripts): IPC probe reports failure
        topt.fail_ipc_probe = True
    if os.environ.get("STENCIL_RCCL_STALL_RANK") is not None:  # rehearses a rank stuck in RCCL creation
        topt.stall_rccl_init_rank = int(os.environ["STENCIL_RCCL_STALL_RANK"])
    return topt


def parse_methods(st, spec: str):
    if spec == "all":
        return st.MethodFlags.All
    m = st.MethodFlags.None_
    for k in spec.split(","):
        m = m | getattr(st.MethodFlags, {"staged": "Staged", "rccl": "Rccl", "colo": "Colocated",
                                         "peer": "PeerCopy", "kernel": "Kernel"}[k])
    return m


def emit(line: dict):
    """Rank 0's JSON line. Printed twice: right after the headline loop (so nothing later -- the transport sweep on
    real links -- can cost it), then again with extra.transports filled in."""
    print(json.dumps(line), flush=True)


def arm_deadline(seconds: float, rank: int):
    """Every rank exits 0 if the sweep is still running `seconds` from now: the headline line is already out, and a
    hung transport entry must end the job, not run it into the driver's limit."""
    import threading

    def fire():
        print(f"[bench] rank {rank}: transport sweep still running after {seconds:.0f} s; abandoning it (the headline "
              f"line was printed before the sweep)", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(0)

    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


class Phases:
    """Wall time of each bench phase (config.phases_s), so the time an N-GPU run spends before its headline line is
    known; `spent()` is the tuning clock the --tune-budget is checked against (agreed over ranks)."""

    def __init__(self):
        self.t = {}
        self.t0 = time.perf_counter()
        self.tune0 = None

    def mark(self, name: str, since: float):
        self.t[name] = round(self.t.get(name, 0.0) + time.perf_counter() - since, 3)

    def tuning_spent(self, env) -> float:
        if self.tune0 is None:
            self.tune0 = time.perf_counter()
        return env.agreed_max(time.perf_counter() - self.tune0)


def exchange_trimean(env, dd, iters: int, xbytes: int) -> dict:
    """The reference's exchange statistic (bin/bench_exchange.cu:39-63): each exchange()+swap() timed on its own
    behind a barrier, the max over ranks per iteration, then the trimean (bin/statistics.cpp: (Q1 + 2 Q2 + Q3) / 4);
    GB/s = aggregate halo bytes over all ranks / trimean."""
    import stencil2_amd as st
    stats = st._C.Statistics()
    for _ in range(iters):
        env.barrier()
        t = time.perf_counter()
        dd.exchange()
        dd.swap()
        env.sync()
        stats.insert(env.agreed_max(time.perf_counter() - t))
    tm = stats.trimean()
    return {"trimean_ms": round(tm * 1e3, 4), "trimean_GBps": round(xbytes / tm / 1e9, 3) if tm > 0 else None,
            "min_ms": round(stats.min() * 1e3, 4)}


RUN_GRAPH_STEPS = 1008  # 56 hipGraph blocks of 18 steps: whole pairs and triples, under prepare()'s 1024-step limit


def run_lengths(steps: int) -> list:
    """The run() calls that make up `steps` timed steps. StencilModel.prepare records a whole run as one graph up to
    1024 steps, so a longer loop is enqueued as runs of RUN_GRAPH_STEPS plus the remainder: the same sweeps in the
    same order as one run(steps), one graph launch per 1008 steps."""
    return [RUN_GRAPH_STEPS] * (steps // RUN_GRAPH_STEPS) + [steps % RUN_GRAPH_STEPS] * (steps % RUN_GRAPH_STEPS > 0)


def run_steps(model, steps: int):
    for k in run_lengths(steps):
        model.run(k)


DUMP_BYTES = 48 << 20  # --dump-outputs: all ranks together
DUMP_SEED = 7


def dump_outputs(torch, model, directory: str, rank: int, world: int) -> dict:
    """--dump-outputs: this rank's interior (z, y, x) as the timed loop left it -> DIR/u_rank<r>.npy (float32). The
    initial condition and the number of steps before this point depend on the arguments alone, so equal arguments give
    equal inputs. A field over this rank's share of DUMP_BYTES is written as a 1-D sample: the cells at the sorted
    flat interior indices numpy.random.default_rng(DUMP_SEED + rank).integers(0, cells, share // 4)."""
    import numpy as np

    u = model.interior(0)
    cells = u.numel()
    keep = DUMP_BYTES // world // 4
    if cells > keep:
        idx = torch.from_numpy(np.sort(np.random.default_rng(DUMP_SEED + rank).integers(0, cells, keep))).to(u.device)
        nz, ny, nx = u.shape
        u = u[idx // (ny * nx), idx // nx % ny, idx % nx]
    a = u.detach().to("cpu", torch.float32).contiguous().numpy()
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"u_rank{rank}.npy")
    np.save(path, a)
    return {"file": path, "shape": list(a.shape), "cells": int(cells), "sampled": bool(cells > keep)}


def main(argv=None):
    args = build_args(argv)
    rc = rank_setup(args.gpus, args.launch_timeout, sys.argv[1:] if argv is None else list(argv))
    if rc is not None:
        return rc
    if not args.cpu:
        _limit_queues_when_sharing()

    import torch
    import torch.distributed as dist

    ph = Phases()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = 0 if args.cpu else torch.cuda.device_count()
    device = local_rank % max(1, ndev)
    if not args.cpu:
        torch.cuda.set_device(device)
    # one rank per GPU: RCCL for the harness barrier/max-reduce. More ranks than GPUs (a rehearsal on a 1-GPU box,
    # ranks sharing the device through HIP IPC) cannot use RCCL, so the harness collectives go over gloo (as --cpu).
    shared = args.cpu or world > ndev
    if world > 1:
        if shared:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
    env = Env(torch, dist, args.cpu, world, "cpu" if shared else "cuda")

    import stencil2_amd as st

    pg = st.init_process_group()
    n = world
    axis_cost = tuple(int(v) for v in args.axis_cost.split(","))
    objective = st.PartitionObjective.MaxLink if args.partition == "maxlink" else st.PartitionObjective.Interface
    grid = weak_grid(st, args.per_gpu, n, args.grid, axis_cost, objective)
    methods = parse_methods(st, args.methods)
    tune = make_tune(st, args)
    tune.x2reserve = args.x2reserve
    ph.mark("startup", ph.t0)

    # Transport self-test (multi-process only, DistributedDomain::set_self_test, run inside realize): a
    # coordinate-encoded field on a small probe domain with the model's radius, placement and transports is exchanged
    # and checked cell by cell on every rank; any wrong halo or error drops Colocated, then Rccl (host-staged), so a
    # scaling run never times silently corrupted halos. An RCCL communicator that fails to form (or never forms:
    # bounded non-blocking creation) falls back to the host-staged path on every rank as well.
    def build(topt, meth, wrap_self=None, shared=None):
        model = st.Jacobi3D(grid, gpus=[device], methods=meth, overlap=args.overlap != "off",
                            auto_overlap=args.overlap == "auto", tune=tune, temporal=args.temporal, group=pg,
                            axis_cost=axis_cost, partition=objective,
                            wrap_self=bool(args.wrap) if wrap_self is None else wrap_self, transport=topt,
                            self_test=bool(args.self_test) and world > 1,
                            interior_align=args.interior_align, backend=st.Backend.Host if args.cpu else None,
                            shared_halo_line=bool(args.shared_halo_line == 1 if shared is None else shared))
        model.init()
        # hipGraph capture + instantiation (no steps run) outside the timed region: the 18-step blocks, and one graph of
        # a whole run(--steps) (the blocks plus the remainder in one launch; the same kernels in the same order)
        model.prepare(sorted(set(run_lengths(args.steps))))
        model.run(args.warmup)
        model.synchronize()
        env.barrier()
        return model

    def timed_run(model, k):
        env.barrier()
        t = time.perf_counter()
        model.run(k)
        model.synchronize()
        return env.agreed_max(time.perf_counter() - t) / k * 1e3

    def release(model):
        """every rank, whether or not it holds a model (the barrier keeps the harness collectives in step)"""
        del model
        import gc
        gc.collect()
        env.barrier()

    # Transport chosen by measurement (N > 1): whole steps, max over ranks, best of two rounds, for Colocated over the
    # three inbox memories and for Rccl (the reference ladder's next rung). A default picked where "xGMI" was local
    # HBM must not decide the first multi-GPU record (reference: per-rung runs,
    # scripts/summit/weak_256n.sh:26-30, ladder src/stencil.cu:163-194). Bounded by --tune-budget.
    topt = make_transport(st, args)
    transport_tuned = None
    model = None
    t_ph = time.perf_counter()
    if world > 1 and args.transport == "auto" and args.tune_steps > 0:
        M = st.MethodFlags
        cands = [("colo_uncached", methods, "uncached"), ("colo_fine", methods, "fine"),
                 ("colo_coarse", methods, "coarse"),
                 ("rccl", M(int(methods) & ~int(M.Colocated)), args.inbox)]
        k = max(2, args.tune_steps // 2 * 2)
        best = None
        transport_tuned = {}
        for name, meth, inbox in cands:
            rec = {}
            if ph.tuning_spent(env) >= args.tune_budget:
                transport_tuned[name] = {"skipped": f"tune budget {args.tune_budget:.0f} s spent"}
                continue
            cand = None
            t_ = None
            try:
                t_ = make_transport(st, args, inbox)
                cand = build(t_, meth)
                rec["realized"] = used_methods(st, cand.domain)
                if cand.domain.rccl_status():
                    rec["rccl_status"] = cand.domain.rccl_status()
                ms = min(timed_run(cand, k), timed_run(cand, k))
                rec["ms"] = round(ms, 4)
            except Exception as e:  # noqa: BLE001 -- a candidate failing on this rank: the others learn it below
                rec["error"] = f"{type(e).__name__}: {str(e)[:200]}"
                ms = float("inf")
            # agreed before any rank-local branch: every rank keeps or releases the same candidate
            failed = env.agreed_max(0.0 if "error" not in rec else 1.0) > 0
            if failed:
                ms = float("inf")
                rec.setdefault("error", "failed on another rank")
            ms = env.agreed_max(ms)
            transport_tuned[name] = rec
            if rank == 0:
                print(f"[bench] transport choice {name}: {rec}", file=sys.stderr, flush=True)
            if not failed and (best is None or ms < best[0]):
                if best is not None:
                    release(best[1])
                best = (ms, cand, name, t_, meth)
            else:
                release(cand)
        if best is None:
            transport_tuned["chosen"] = "fixed (every candidate failed or was skipped)"
        else:
            _, model, chosen, topt, methods = best
            transport_tuned["chosen"] = chosen
        ph.mark("transport_warmup", t_ph)
    if model is None:
        t_b = time.perf_counter()
        model = build(topt, methods)
        ph.mark("build", t_b)
    methods = model.domain.methods()
    preflight = model.domain.self_test_report() or "skipped"
    colo = model.domain.exchange_bytes_for_method(st.MethodFlags.Colocated) > 0

    # overlapped vs whole-region sweeps (remote halos only): all run, the fastest (max over ranks, best of two
    # rounds) is kept for the timed loop -- part of the warm-up, every rank takes the same decision
    overlap_tuned = None
    t_ph = time.perf_counter()
    if args.overlap == "auto" and args.tune_steps > 0 and model.can_toggle_overlap():
        best = {}
        # whole-region candidates (mode 0) run fused triples where the model can (temporal 3): probe and time whole
        # triples and pairs alike (multiples of 6 steps)
        sweep = 6 if args.temporal >= 3 else 2
        k = max(sweep, args.tune_steps // sweep * sweep)
        r0 = args.x2reserve
        # (mode, CUs left to the transports, co-located copy): mode 1 = slabs beside the sweep, 2 = slabs after
        # it, 0 = whole-region sweeps (fused triples where possible), 3 = pipelined whole-region pairs, 4 = pipelined
        # triples; copy "s" = pack kernel stores into the peer inbox, "e" = DMA engine copy (the transports then need
        # fewer CUs: also tried with a quarter of the reserve). Whole-region first: the default if the budget ends
        copies = ["s", "e"] if colo and args.colo_copy == "auto" else ["e" if args.colo_copy == "engine" else "s"]
        cands = []
        for cp in copies:
            cands.append((0, r0, cp))
            # modes 3 / 4 (pipelined: the next exchange gated on the sweep's published boundary planes) need the
            # pack-kernel stores
            if cp == "s" and model.can_pipeline_triples():
                cands += [(4, r0, cp), (4, max(1, r0 // 2), cp), (4, 2 * r0, cp)]
            if cp == "s" and model.can_pipeline():
                cands += [(3, r0, cp), (3, max(1, r0 // 2), cp), (3, 2 * r0, cp)]
            cands += [(1, r0, cp), (1, max(1, r0 // 2), cp), (1, 2 * r0, cp), (2, r0, cp)]
            if cp == "e":
                cands.append((1, max(1, r0 // 4), cp))

        def apply(c):
            model.domain.set_colo_copy(topt.Copy.Engine if c[2] == "e" else topt.Copy.Store)
            model.set_overlap_mode(c[0])
            model.set_comm_reserve(c[1])

        skip, over = set(), []
        for c in cands + cands:
            if c in skip:
                continue
            if ph.tuning_spent(env) >= args.tune_budget:
                if c not in best:
                    over.append(c)
                continue
            apply(c)
            model.run(sweep)
            model.synchronize()
            # a short probe first: a candidate far slower than the best so far (ranks sharing one GPU: DMA-engine
            # copies beside overlapped sweeps ran at ~0.8 s per step, profiles/r3/check2) is not given full rounds
            ref = min(best.values(), default=float("inf"))
            t = timed_run(model, sweep)
            if t > 4 * ref:
                skip.add(c)
                best[c] = min(best.get(c, float("inf")), t)
            else:
                best[c] = min(best.get(c, float("inf")), t, timed_run(model, k))
            if rank == 0:
                print(f"[bench] overlap choice {c}: {best[c]:.4f} ms/step{' (skipped)' if c in skip else ''}",
                      file=sys.stderr, flush=True)
        timed = [c for c in cands if c in best]
        choice = min(timed, key=lambda c: best[c]) if timed else (model.overlap_mode(), r0, copies[0])
        apply(choice)
        model.run(sweep)
        model.synchronize()
        env.barrier()
        overlap_tuned = {"mode": choice[0], "reserve": choice[1], "colo_copy": "engine" if choice[2] == "e" else "store",
                         "triples": bool(model.temporal_triples()),
                         **{f"m{c[0]}_r{c[1]}_{c[2]}_ms": round(best[c], 4) for c in timed}}
        if over:
            overlap_tuned["skipped_by_budget"] = [f"m{c[0]}_r{c[1]}_{c[2]}" for c in over]
        ph.mark("overlap_warmup", t_ph)

    # Fused-triple schedule chosen by measurement: the host plan's step estimate (sphere weight, leftover plan) is a
    # model; each candidate is recorded (prepare) and timed over whole 18-step blocks, best of --schedule-rounds
    # interleaved rounds, max over ranks (the same choice on every rank). Launch geometry only: every candidate is
    # bitwise the same computation. Bounded by --tune-budget.
    schedule_tuned = None
    t_ph = time.perf_counter()
    if args.tune_steps > 0 and args.schedule_rounds > 0 and model.temporal_triples() and not args.cpu:
        scands = [(0.45, 3), (0.3, 3), (0.6, 3), (0.6, 1), (0.45, 2)]
        best, over = {}, []
        for _ in range(args.schedule_rounds):
            for c in scands:
                if ph.tuning_spent(env) >= args.tune_budget:
                    if c not in best and c not in over:
                        over.append(c)
                    continue
                model.set_triple_schedule(c[0], c[1], 0)
                model.prepare([18])
                model.run(18)
                model.synchronize()
                best[c] = min(best.get(c, float("inf")), timed_run(model, 18))
        choice = min(best, key=best.get) if best else scands[0]
        model.set_triple_schedule(choice[0], choice[1], 0)
        model.prepare(sorted(set(run_lengths(args.steps))))
        model.run(args.warmup)
        model.synchronize()
        env.barrier()
        tune.x3sphw, tune.x3left = choice
        schedule_tuned = {"x3sphw": choice[0], "x3left": choice[1],
                          **{f"sphw{c[0]}_left{c[1]}_ms": round(v, 4) for c, v in best.items()}}
        if over:
            schedule_tuned["skipped_by_budget"] = [f"sphw{c[0]}_left{c[1]}" for c in over]
        if rank == 0:
            print(f"[bench] triple schedule {choice}: " + ", ".join(f"{c}: {v:.4f}" for c, v in best.items()),
                  file=sys.stderr, flush=True)
        ph.mark("schedule_warmup", t_ph)

    # ---- the timed loop: exactly --steps steps, bracketed by a barrier + device synchronize on both sides ----
    env.barrier()
    t0 = time.perf_counter()
    run_steps(model, args.steps)  # every step is enqueued; whole blocks of steps replay as one hipGraph where possible
    model.synchronize()
    env.sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    elapsed = env.agreed_max(elapsed)
    ph.mark("timed_loop", t0)
    cells = grid[0] * grid[1] * grid[2]
    gcells = cells * args.steps / elapsed / 1e9

    dumped = None
    if args.dump_outputs:
        t_ph = time.perf_counter()
        dumped = dump_outputs(torch, model, args.dump_outputs, rank, world)
        ph.mark("dump_outputs", t_ph)

    # --full: exchange-only loops on the same decomposition (halo-exchange GB/s, bench_exchange definition)
    dd = model.domain
    xbytes = int(dd.exchange_bytes_for_method(st.MethodFlags.All))
    xrec = {}
    if args.full:
        t_ph = time.perf_counter()
        dd.set_comm_max_blocks(0)  # the exchange alone may use the whole GPU (the overlapped steps confine it to 8 CUs)
        colo_log = colo and topt.completion != topt.Completion.StreamOp and not args.cpu
        xrec = time_exchanges(env, dd, args.exchange_iters, xbytes, log=colo_log)
        xrec.update(exchange_trimean(env, dd, args.exchange_iters, xbytes))
        ph.mark("exchange_loops", t_ph)

    pdim = dd.placement_dim()
    wrap_axes = "".join(c for i, c in enumerate("xyz") if model.wrap_axes() >> i & 1) or "none"
    model_cfg = {
        "decomposition": f"{pdim.x}x{pdim.y}x{pdim.z}", "methods": st.methods_to_string(methods), "preflight": preflight,
        "overlap": model.overlapping(), "overlap_mode": model.overlap_mode(), "overlap_tuned": overlap_tuned,
        "schedule_tuned": schedule_tuned,
        "transport_tuned": transport_tuned, "interior_align": args.interior_align,
        "shared_halo_line": args.shared_halo_line == 1,
        "temporal": 3 if model.temporal_triples() else (2 if model.temporal_blocking() else 1),
        "wrap_axes": wrap_axes, "backend": "host" if args.cpu else "device", "tune": tune_record(tune),
        "transport": {"inbox": str(dd.transport_options().inbox).split(".")[-1].lower(),
                      "colo_copy": str(dd.transport_options().colo_copy).split(".")[-1].lower(),
                      "completion": args.completion, "fuse_flags": bool(args.fuse_flags)},
        "phases_s": ph.t,
    }
    mode_tuned = model.overlap_mode()
    del dd
    release(model)
    model = None

    out = {
        "metric": "Jacobi3D Gcells/s (512^3/GPU weak scaling; halo-exchange GB/s in extra)",
        "value": round(gcells, 3),
        "unit": "Gcells/s",
        "n_gpus": n,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic (reference Jacobi3D initial condition: 0.5 + hot/cold spheres)",
        "config": {"model": "jacobi3d", "global_batch": cells, "seq_len": max(grid),
                   "grid": list(grid), "grid_rule": args.grid, "partition": args.partition, "per_gpu": args.per_gpu,
                   "radius": 1, "parallelism": f"domain-decomp{n}",
                   **model_cfg,
                   "build": st.build_info()["git_sha"]},
        "extra": {"full": args.full, "dumped": dumped,
                  "halo_exchange_GBps": xrec.get("GBps"), "halo_exchange_stream_GBps": xrec.get("stream_GBps"),
                  "halo_exchange_trimean_GBps": xrec.get("trimean_GBps"),
                  "halo_bytes_per_exchange": xbytes, "exchange_ms": xrec.get("exchange_ms"),
                  "exchange_trimean_ms": xrec.get("trimean_ms"),
                  "gcells_per_gpu": round(gcells / n, 3), "colo_kernels_us": xrec.get("colo_kernels_us"),
                  "gcells_with_exchange": None, "with_exchange": None,
                  "transports": "pending" if args.full and (args.transport_sweep == "on" or
                                                            (args.transport_sweep == "auto" and world > 1)) else None},
    }

    # BASELINE config 2 as the reference times it (bin/jacobi3d.cu:265-346: exchange() every iteration): the same
    # steps with every halo copied -- the intra-GPU pack/unpack (same-GPU copy-plan kernel) plus the compute kernels
    # (fused triples reading x from 3-deep halos where the layout allows). A failure here costs this entry, not the
    # headline
    if args.full and (args.with_exchange == "on" or (args.with_exchange == "auto" and wrap_axes != "none")):
        t_ph = time.perf_counter()
        m2 = None
        try:
            m2 = build(topt, methods, wrap_self=False, shared=args.shared_halo_line != 0)
            if overlap_tuned is not None and m2.can_toggle_overlap():
                # the tuned mode only where this model supports it (pipelined modes need the gate / the triples)
                md = mode_tuned
                if (md == 4 and not m2.can_pipeline_triples()) or (md == 3 and not m2.can_pipeline()):
                    md = 0
                m2.set_overlap_mode(md)
                m2.set_comm_reserve(overlap_tuned["reserve"])
                m2.run(6)
                m2.synchronize()
            env.barrier()
            t = time.perf_counter()
            run_steps(m2, args.steps)
            m2.synchronize()
            env.sync()
            el = env.agreed_max(time.perf_counter() - t)
            out["extra"]["with_exchange"] = {
                "gcells": round(cells * args.steps / el / 1e9, 3), "ms_per_step": round(el / args.steps * 1e3, 4),
                "wrap_axes": "".join(c for i, c in enumerate("xyz") if m2.wrap_axes() >> i & 1) or "none",
                "temporal": 3 if m2.temporal_triples() else (2 if m2.temporal_blocking() else 1),
                "overlap_mode": m2.overlap_mode(),
                "shared_halo_line": bool(m2.domain.domain(0).shared_halo_line()),
                "halo_bytes_per_exchange": int(m2.domain.exchange_bytes_for_method(st.MethodFlags.All))}
            out["extra"]["gcells_with_exchange"] = out["extra"]["with_exchange"]["gcells"]
        except Exception as e:  # noqa: BLE001
            out["extra"]["with_exchange"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        release(m2)
        ph.mark("with_exchange", t_ph)

    if rank == 0:
        emit(out)  # line 1: the headline, before anything that could hang

    if out["extra"]["transports"] == "pending":
        t_ph = time.perf_counter()
        timer = arm_deadline(args.sweep_deadline, rank)
        out["extra"]["transports"] = transport_sweep(st, env, args, world, rank, device, ndev, axis_cost, objective,
                                                     topt, methods)
        timer.cancel()
        ph.mark("sweep", t_ph)
        if rank == 0:
            emit(out)  # line 2: the same headline with the sweep
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
