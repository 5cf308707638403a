"""Field algebra on the device (csrc/src/kernels/field_axpby.hip): the row kernel of the aligned vector layout over
rows shorter than a chunk, rows off the chunk grid, exactly one wave-row with and without an extra cell, aliased
operands, sub-regions with every other byte checked, forced grids and non-temporal stores; the one-thread-per-cell
kernel on the unpadded and halo-aligned layouts; the stats fused into the same pass; stream order behind star_apply;
several sub-domains per GPU, two ranks on one GPU and the StarCG solver. test_algebra.py runs the same cases
(algebra_cases.py) on the host backend."""
import os

import pytest
import torch

import algebra_cases as cases
import reduce_cases as rc
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "algebra_worker.py")
DTYPES = [torch.float32, torch.float64]


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_bitwise_shapes(st, dev, case):
    """every shape has the padded (aligned) layout, so the row kernel is the one launched"""
    cases.case_shape(st, dev, case[0], case[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size", cases.ALIAS_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(cases.ALIASES))
def test_aliasing(st, dev, name, size, dtype):
    cases.case_alias(st, dev, size, dtype, name)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.regions((37, 11, 9))))
def test_untouched_bytes(st, dev, name, dtype, stats):
    cases.case_region(st, dev, name, dtype, stats)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.rc.LAYOUTS))
def test_layouts(st, dev, name, dtype):
    cases.case_layout(st, dev, name, dtype)


@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, dev, es):
    cases.case_opaque(st, dev, es)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,max_blocks", cases.FORCED)
def test_forced_grids(st, dev, size, max_blocks, dtype):
    cases.case_forced_grid(st, dev, size, dtype, max_blocks)


def test_several_blocks_by_default(st, dev):
    """(131, 17, 33) has 561 (row, plane) items: the automatic grid is more than one block, with and without stats"""
    r = cases.Runner(st, dev, cases.RANDOM_SIZE, torch.float32)
    for stats in (False, True):
        _, info, _ = r.run(1.3, 2.9, ("a", True), ("b", True), ("c", False), stats=stats)
        assert info["path"] == "fast" and info["items"] == 17 * 33 and 1 < info["blocks"] <= 17 * 33, info


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_stats_exact(st, dev, case, two):
    cases.case_stats_exact(st, dev, case[0], case[1], two)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size", [(37, 11, 9), (257, 3, 2), (131, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_nontemporal_stores(st, dev, size, dtype, two):
    """the nt-hinted 16-B stores write the same bytes and return the same exact stats"""
    cases.case_stats_exact(st, dev, size, dtype, two, nontemporal=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_random_within_summation_bound(st, dev, dtype):
    cases.case_stats_random(st, dev, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_nonfinite(st, dev, dtype):
    cases.case_stats_nonfinite(st, dev, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_stats_repeatable_bits(st, dev, dtype):
    cases.case_stats_repeatable(st, dev, dtype)


def test_stream_order_behind_star_apply(st, dev):
    """star_apply on a stream, then field_axpby with stats reading next on the same stream with no synchronization in
    between: it combines the new next (integer weights and data: exact), not the NaN the buffer held before"""
    from stencil2_amd.ops import field_axpby, star_apply, star_step_reference, star_weights
    size = cases.RANDOM_SIZE
    dd, qa, qb, _ = rc.make_domain(st, dev, size, torch.float32)
    rc.poison(dd, [qa, qb])
    A = rc.exact_field(size, 21)
    rc.put(dd, qa, True, A.float())
    dd.exchange()
    w = star_weights(1, 2.0, [1.0, -1.0], [3.0, 1.0], [-2.0, 1.0])
    want = 2 * star_step_reference(A.float(), w).to(torch.int64) - 3 * A
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    star_apply(dd, 0, qa, w, stream=s.cuda_stream)
    got = field_axpby(dd, 0, qb, 2, qa, -3, qa, x_curr=False, y_curr=True, stream=s.cuda_stream, stats=True)
    rc.check_exact(got, rc.expect_exact(want), "2 next - 3 curr after star_apply")
    assert cases.same_bits(cases.get(dd, qb, True, torch.float32), want.float())


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


@pytest.mark.parametrize("gpus", [[0], [0, 0, 0]], ids=["one", "three"])
def test_sub_domains(st, dev, gpus):
    cases.case_dd(st, dev, gpus)


def test_two_ranks_one_gpu():
    """dd.axpby with stats and StarCG on two ranks sharing GPU 0: exact values on every rank, the random field's
    struct and the solver's (iters, relres) bitwise identical on both"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for code, out in outs:
        assert code == 0, out[-3000:]
    assert all("axpby bad 0 " in out and " of 2 " in out and "'fast'" in out for _, out in outs), outs
    for prefix in ("hex ", "cg iters "):
        lines = [[ln for ln in out.splitlines() if ln.startswith(prefix)] for _, out in outs]
        assert len(lines[0]) == 1 and lines[0] == lines[1], lines


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.CG_CASES))
def test_cg(st, dev, name, dtype):
    cases.case_cg(st, dev, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_cg_sub_domains(st, dev, dtype):
    cases.case_cg(st, dev, "helmholtz_walls", dtype, gpus=(0, 0))


def test_cg_limits(st, dev):
    cases.case_cg_limits(st, dev)


def test_wall_second_order(st, dev):
    cases.case_wall_order(st, dev)
