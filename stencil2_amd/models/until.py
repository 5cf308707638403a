"""run_until: advance a model until the change made by one step falls below a tolerance.

Shared by StarStencil3D and StencilModel (Jacobi3D, AstarothSim). The model advances in blocks of `check_every` steps
(`run(check_every - 1)`, then one single `step()`), synchronizes, and reduces curr - next over the compute regions of
every quantity (`DistributedDomain.reduce`, collective: every rank sees the same value and stops at the same check).
After a single step and its swap, next holds the state before that step: a single step writes only the compute region
of its destination buffer, the exchange and the halo-forwarding kernels write halos only, and nothing else stores into
the source buffer. That holds for every configuration of the models (forwarding, overlapped, in-kernel wrap, fused
pairs / triples with a single-step remainder), so none is refused; the value is the change of the block's last step.
"""
from __future__ import annotations

import math

NORMS = (1, 2, "inf")


def _combine(stats, norm):
    """one value from the per-quantity FieldStats: max of the inf-norms, sum of the 1-norms, root of the summed squares"""
    if norm == "inf":
        return max(s.linf for s in stats)
    if norm == 1:
        return math.fsum(s.l1 for s in stats)
    return math.sqrt(math.fsum(s.sum_sq for s in stats))


def run_until(model, reduce, quantities, tol, max_iters, check_every=10, norm="inf"):
    """(iters_done, value): see the models' run_until. `reduce(q)` returns the FieldStats of curr(q) - next(q)."""
    if norm not in NORMS:
        raise ValueError(f"norm must be 1, 2 or 'inf', not {norm!r}")
    check_every, max_iters = int(check_every), int(max_iters)
    if check_every < 1:
        raise ValueError(f"check_every must be >= 1, not {check_every}")
    if max_iters < 0:
        raise ValueError(f"max_iters must be >= 0, not {max_iters}")
    done, value = 0, math.inf
    while done < max_iters:
        n = min(check_every, max_iters - done)
        if n > 1:
            model.run(n - 1)
        model.step()
        model.synchronize()
        done += n
        stats = [reduce(q) for q in quantities]
        bad = sum(s.nonfinite for s in stats)
        if bad > 0:
            raise FloatingPointError(f"run_until: {bad} non-finite cells in the change of step {done}")
        value = _combine(stats, norm)
        if value < tol:
            break
    return done, value
