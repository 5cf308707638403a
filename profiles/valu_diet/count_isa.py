#!/usr/bin/env python3
"""Static instruction counts of the steady z-step loop of stencil7x3_wrap_kernel in a gfx950 .s file.

usage: count_path.py FILE.s MANGLED_KERNEL_NAME [--spheres]

Walks the role-3 (output rows) steady loop of the first march the file holds along the path a wave normally takes:
the rare tiny-sum branches (s_cbranch_execnz / execz) and the loop exits (s_cbranch_vccnz, long forward s_cbranch_scc1)
are not taken, the short forward s_cbranch_scc1 that skips a level's per-cell sphere tests is taken unless --spheres
is given. The loop starts behind the first barrier that follows the first nontemporal (or plain) output store and
ends when the walk returns there. Prints the counts per loop iteration (4 unrolled z steps) and per z step, the
vmcnt waits and the order of the memory instructions of one step."""
import re
import sys
from collections import Counter


def parse(path, name):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels, insts = {}, []
    for l in lines[start:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        t = l.strip()
        if not t or t.startswith(";") or t.startswith("."):
            continue
        t = t.split(";")[0].strip()
        insts.append((t.split()[0], t))
    return labels, insts


def klass(op, t):
    if "wave_ro" in t or "row_" in t or "quad_perm" in t:
        return "DPP"
    if op.startswith("v_pk_mov") or op.startswith("v_mov"):
        return "v_mov / v_pk_mov"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("v_min") or op.startswith("v_max"):
        return "v_min*"
    if op.startswith("v_cmp"):
        return "v_cmp*"
    if op.startswith("v_pk_"):
        return "v_pk_add/mul/fma"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("ds_"):
        return "ds_*"
    if op.startswith("buffer_load") or op.startswith("global_load"):
        return "VMEM load"
    if op.startswith("global_store") or op.startswith("buffer_store"):
        return "VMEM store"
    if op == "s_barrier":
        return "s_barrier"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branches"
    if op.startswith("scratch_"):
        return "scratch"
    return "other SALU"


def main():
    path, name = sys.argv[1], sys.argv[2]
    spheres = "--spheres" in sys.argv
    labels, insts = parse(path, name)
    st = next(i for i, (op, t) in enumerate(insts) if op.startswith("global_store_dwordx4"))
    start = next(i for i in range(st, len(insts)) if insts[i][0] == "s_barrier") + 1
    pc, seen, walk = start, set(), []
    while True:
        if pc in seen:
            break
        seen.add(pc)
        op, t = insts[pc]
        walk.append((pc, op, t))
        nxt = pc + 1
        if op == "s_branch":
            nxt = labels[t.split()[-1]]
        elif op == "s_cbranch_scc1" or op == "s_cbranch_scc0":
            tgt = labels[t.split()[-1]]
            if 0 < tgt - pc <= 80 and not spheres:
                nxt = tgt
        pc = nxt
        if pc == start:
            break
    c = Counter(klass(op, t) for _, op, t in walk)
    nb = c["s_barrier"]
    valu = sum(v for k, v in c.items() if k in ("DPP", "v_mov / v_pk_mov", "v_cndmask", "v_min*", "v_cmp*",
                                                 "v_pk_add/mul/fma", "other VALU"))
    print(f"{name}\n  steady loop: {len(walk)} instructions on the usual path"
          f"{' with all sphere tests' if spheres else ''}, {nb} z steps (barriers) per iteration, "
          f"instruction indices {min(p for p, _, _ in walk)}..{max(p for p, _, _ in walk)}")
    print(f"  {'class':22s} {'per iteration':>14s} {'per z step':>11s}")
    order = ["DPP", "v_mov / v_pk_mov", "v_cndmask", "v_min*", "v_cmp*", "v_pk_add/mul/fma", "other VALU"]
    for k in order:
        print(f"  {k:22s} {c[k]:14d} {c[k] / nb:11.2f}")
    print(f"  {'VALU total':22s} {valu:14d} {valu / nb:11.2f}")
    for k in ["ds_*", "VMEM load", "VMEM store", "s_barrier", "s_waitcnt", "branches", "other SALU", "scratch"]:
        print(f"  {k:22s} {c[k]:14d} {c[k] / nb:11.2f}")
    waits = Counter(t for _, op, t in walk if op == "s_waitcnt" and "vmcnt" in t)
    print("  vmcnt waits:", dict(waits))
    print("  stores nt:", sum(1 for _, op, t in walk if op.startswith("global_store") and t.endswith(" nt")))
    # order of memory instructions in the first step
    seq = []
    for _, op, t in walk:
        if op.startswith("buffer_load") or op.startswith("global_store") or op.startswith("ds_") or \
                (op == "s_waitcnt" and "vmcnt" in t) or op == "s_barrier":
            seq.append(op if op != "s_waitcnt" else t.replace("s_waitcnt ", ""))
        if op == "s_barrier" and len([s for s in seq if s == "s_barrier"]) == 1 and seq[0] != "s_barrier":
            break
    print("  memory order of one step:", " ".join(seq))


main()
