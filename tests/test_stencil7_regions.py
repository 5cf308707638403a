"""The single 7-point step on the host backend (host_apply and the host path of stencil7_apply_regions in
csrc/src/kernels/stencil7.hip) through the check of stencil7_cases.py: the region bitwise equal to the torch CPU oracle,
every other byte of the `next` allocation untouched; and the oracle itself against its fp64 evaluation.
test_gpu_stencil7_regions.py runs the device's share of the cases."""
import pytest
import torch

import stencil7_cases as cases
from star_cases import sub_regions

F32, F64 = torch.float32, torch.float64
SUBS = sorted(sub_regions(cases.SUB_SIZE))


@pytest.fixture
def host(st):
    return st.Backend.Host


@pytest.fixture(scope="module", autouse=True)
def _drop_domains():
    yield
    cases.drop_domains()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_oracle_against_fp64(kind):
    worst = cases.case_oracle_against_fp64(kind)
    print(f"fp32 oracle ({kind}) within {worst:.3e} of the fp64 evaluation (bound {2.0 ** -22:.3e})")


def test_fill_value_is_no_stencil_result(st, host):
    for dtype in cases.DTYPES:
        cases.fill_word(cases.domain(st, host, cases.SUB_SIZE, "face1", dtype))


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", SUBS)
def test_host_apply_sub_regions(st, host, name, kind, dtype):
    cases.case_single_sub_region(st, host, name, cases.DEFAULT, kind, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_host_apply_whole_region_and_parity(st, host, kind, dtype):
    cases.case_single_parity(st, host, cases.DEFAULT, kind, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_host_apply_regions_sub_regions(st, host, kind, dtype):
    """the seven sub-regions one at a time through stencil7_apply_regions (an empty one among two)"""
    from stencil2_amd.ops import stencil7_apply_regions
    dom = cases.domain(st, host, cases.SUB_SIZE, "face1", dtype)
    ref = cases.oracle(cases.SUB_SIZE, dtype, kind)
    subs = sub_regions(cases.SUB_SIZE)
    for name in SUBS:
        regions = [subs[name], subs["empty"]]
        call = lambda: stencil7_apply_regions(dom.dd, 0, dom.q, [dom.rect(lo, hi) for lo, hi in regions],  # noqa: E731
                                              cases.kind_of(kind), spheres=kind == "jacobi")
        cases.run_check(dom, call, regions, ref, what=f"host regions {name}")


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", ["shell1", "shell3", "width7and8", "many17"])
def test_host_apply_regions_sets(st, host, name, kind, dtype):
    cases.case_single_regions(st, host, name, kind, dtype)


def test_host_refusals(st, host):
    cases.case_single_refusals(st, host)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("stencil7_apply", "stencil7_apply_regions", "stencil7_wrappable_axes", "stencil7x2_apply_regions",
                 "stencil7x2_apply_exterior", "stencil7x2_wrappable_axes"):
        assert hasattr(ops, name) and hasattr(st._C, name), name
    assert hasattr(st._C.LocalDomain, "buffer_to_host")
