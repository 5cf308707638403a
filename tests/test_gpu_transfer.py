"""Grid transfer on the device (csrc/src/kernels/grid_transfer.hip): the chunk kernels of the aligned vector layout
over rows of one chunk or less, rows off the chunk grid, rows longer than a wave's chunks, more rows than a block
takes and z-march seams; fine sub-regions that start and end on odd cells; add aliased with dst, another quantity or
absent; the one-thread-per-cell kernels on the unpadded layout; two sub-domains cut along each axis; walls whose
composed edge and corner ghost cells are consumed; subnormal data; every refusal. test_transfer.py runs the same
cases (transfer_cases.py) on the host backend."""
import pytest
import torch

import transfer_cases as cases

pytestmark = pytest.mark.gpu
DTYPES = cases.DTYPES


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("size", cases.SHAPES, ids=cases.shape_id)
def test_bitwise_shapes(st, dev, size, dtype):
    """every shape has the padded (aligned) layout: Pair asserts path == "fast" for every launch"""
    cases.case_shape(st, dev, size, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_march_seams(st, dev, dtype):
    cases.case_shape(st, dev, cases.MARCH[0], dtype, zchunk=cases.MARCH[1])


def test_default_march_has_seams(st, dev):
    """40 coarse planes under the z chunk the launch chooses: several items per coarse row, four waves per block"""
    p = cases.Pair(st, dev, (16, 8, 80), torch.float32)
    (info,) = p.prolong(add=("a", True))
    assert info["path"] == "fast" and 4 <= info["zchunk"] < 40 and info["items"] == 4 * -(-40 // info["zchunk"]), info
    assert info["blocks"] == -(-info["items"] // 4), info


@pytest.mark.parametrize("add", sorted(cases.ADDS))
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.FINE_REGIONS))
def test_prolong_regions(st, dev, name, dtype, add):
    cases.case_fine_region(st, dev, name, dtype, add)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("name", sorted(cases.COARSE_REGIONS))
def test_restrict_regions(st, dev, name, dtype):
    cases.case_coarse_region(st, dev, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_unpadded_layout(st, dev, dtype):
    """set_padding(False): Pair asserts path == "generic" for every launch"""
    cases.case_unpadded(st, dev, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("axis", sorted(cases.CUTS))
def test_two_sub_domains(st, dev, axis, dtype):
    cases.case_cut(st, dev, axis, dtype)


@pytest.mark.parametrize("gpus", [(0,), (0, 0)], ids=["one", "two"])
@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_mixed_walls(st, dev, dtype, gpus):
    cases.case_walls(st, dev, dtype, gpus)


@pytest.mark.parametrize("dtype", DTYPES, ids=cases.dtype_id)
def test_subnormal_data(st, dev, dtype):
    cases.case_tiny(st, dev, dtype)


def test_stream_order(st, dev):
    """restriction and prolongation enqueued on one side stream with no synchronization in between: the prolongation
    of the restricted field sees the restriction's stores"""
    from stencil2_amd.ops import prolong_apply, prolong_reference, restrict_apply, restrict_reference
    import reduce_cases as rc
    p = cases.Pair(st, dev, (64, 16, 16), torch.float32)
    qa, qb, qc = p.q["a"][1], p.q["b"][1], p.q["c"][1]
    F = cases.field(p.fsize, torch.float32, 5)
    rc.put(p.fine, qa, True, F)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    restrict_apply(p.fine, p.coarse, 0, qa, qc, stream=s.cuda_stream)
    s.synchronize()
    p.coarse.exchange()
    prolong_apply(p.coarse, p.fine, 0, qc, qb, add=qa, stream=s.cuda_stream)
    restrict_apply(p.fine, p.coarse, 0, qb, qc, dst_curr=False, stream=s.cuda_stream)
    s.synchronize()
    want = prolong_reference(restrict_reference(F), add=F)
    got = p.fine.interior(p.fine.curr(0, qb), 0).cpu()
    assert torch.equal(got, want)
    assert torch.equal(p.coarse.interior(p.coarse.next(0, qc), 0).cpu(), restrict_reference(want))


def test_refusals(st, dev):
    """every refusal is raised on the host before any launch"""
    cases.case_refusals(st, dev)
    cases.case_backends_differ(st)
