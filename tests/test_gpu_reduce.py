"""Field reductions on the device (csrc/src/kernels/field_reduce.hip): the row kernel of the aligned vector layout
over rows shorter than a chunk, rows off the chunk grid, exactly one wave-row with and without an extra cell, forced
grids, sub-regions and layouts; the one-thread-per-cell kernel on the unpadded and halo-aligned layouts; stream order
behind star_apply; several sub-domains per GPU, two ranks on one GPU and the models' run_until. test_reduce.py runs the
same cases (reduce_cases.py) on the host backend."""
import os

import pytest
import torch

import reduce_cases as cases
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "reduce_worker.py")


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("a_curr,b_curr", cases.OPERANDS, ids=["curr-next", "next-curr"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("case", cases.SHAPE_CASES, ids=cases.shape_id)
def test_exact_shapes(st, dev, case, two, a_curr, b_curr):
    """every shape has the padded (aligned) layout, so the row kernel is the one launched"""
    cases.case_exact(st, dev, case[0], case[1], two, a_curr, b_curr)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_two_buffers_of_one_quantity(st, dev, dtype):
    cases.case_exact(st, dev, (37, 11, 9), dtype, True, same_quantity=True)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size,max_blocks", cases.FORCED)
def test_forced_grids(st, dev, size, max_blocks, dtype, two):
    cases.case_forced_grid(st, dev, size, dtype, two, max_blocks)


def test_several_blocks_by_default(st, dev):
    """(131, 17, 33) has 561 (row, plane) items: the automatic grid is more than one block"""
    dd, qa, _, _ = cases.make_domain(st, dev, cases.RANDOM_SIZE, torch.float32)
    info = cases.field_reduce_launch_info(dd, 0, qa)
    assert info["path"] == "fast" and info["items"] == 17 * 33 and 1 < info["blocks"] <= 17 * 33, info


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.sub_regions((37, 11, 9))))
def test_sub_regions(st, dev, name, dtype, two):
    lo, hi = cases.sub_regions((37, 11, 9))[name]
    cases.case_exact(st, dev, (37, 11, 9), dtype, two, lo=lo, hi=hi)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.LAYOUTS))
def test_layouts(st, dev, name, dtype, two):
    cases.case_layout(st, dev, name, dtype, two)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("es", [4, 8])
def test_opaque_elements(st, dev, es, two):
    cases.case_opaque(st, dev, es, two)


@pytest.mark.parametrize("only_nan", [False, True], ids=["nan-inf", "nan"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_nonfinite_cells(st, dev, dtype, two, only_nan):
    cases.case_nonfinite(st, dev, dtype, two, only_nan)


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_random_within_summation_bound(st, dev, dtype, two):
    cases.case_random(st, dev, dtype, two)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
def test_repeatable_bits(st, dev, dtype):
    cases.case_repeatable(st, dev, dtype)


def test_stream_order_behind_star_apply(st, dev):
    """star_apply on a stream, then the reduction of next on the same stream with no synchronization in between: it
    sees the new next (integer weights and data: exact), not the NaN the buffer held before"""
    from stencil2_amd.ops import field_reduce, star_apply, star_step_reference, star_weights
    size = cases.RANDOM_SIZE
    dd, qa, qb, _ = cases.make_domain(st, dev, size, torch.float32)
    cases.poison(dd, [qa, qb])
    A = cases.exact_field(size, 21)
    cases.put(dd, qa, True, A.float())
    dd.exchange()
    w = star_weights(1, 2.0, [1.0, -1.0], [3.0, 1.0], [-2.0, 1.0])
    want = star_step_reference(A.float(), w).to(torch.int64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    star_apply(dd, 0, qa, w, stream=s.cuda_stream)
    got = field_reduce(dd, 0, qa, curr=False, stream=s.cuda_stream)
    cases.check_exact(got, cases.expect_exact(want), "next after star_apply")


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)


@pytest.mark.parametrize("gpus", [[0], [0, 0, 0]], ids=["one", "three"])
def test_sub_domains(st, dev, gpus):
    cases.case_dd_exact(st, dev, gpus)


def test_two_ranks_one_gpu():
    """dd.reduce on two ranks sharing GPU 0: exact values on every rank, the random field's struct bitwise identical"""
    outs = run_ranks(2, WORKER, env_extra={"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20"},
                     timeout=100)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("reduce bad 0 " in out and " of 2 " in out and "'fast'" in out for _, out in outs), outs
    hexes = [[ln for ln in out.splitlines() if ln.startswith("hex ")] for _, out in outs]
    assert len(hexes[0]) == 1 and hexes[0] == hexes[1], hexes


def test_run_until_star(st, dev):
    cases.case_run_until_star(st, dev)


def test_run_until_star_sub_domains(st, dev):
    cases.case_run_until_star(st, dev, gpus=(0, 0))


def test_run_until_jacobi(st, dev):
    cases.case_run_until_jacobi(st, dev)


def test_run_until_jacobi_forwarding(st, dev):
    """halo forwarding: the kernels store into the neighbours' halos of next, never into its compute region"""
    cases.case_run_until_jacobi(st, dev, forward=True)


@pytest.mark.parametrize("kw", [dict(temporal=2), dict(temporal=3), dict(overlap=True, auto_overlap=False),
                                dict(wrap_self=False), dict(use_graph=False), dict(temporal=2, wrap_self=False)],
                         ids=["temporal2", "temporal3", "overlapped", "halos-copied", "no-graph", "temporal2-halos-copied"])
def test_run_until_jacobi_configurations(st, dev, kw):
    """temporal = 2 / 3 (run(check_every - 1) fuses steps where the kernels take this sub-domain; the block's last step
    is always single), overlapped steps, every halo copied instead of wrapped in-kernel, no hipGraph replay: the single
    step that ends a block leaves the state before it in next"""
    cases.case_run_until_jacobi(st, dev, **kw)
