"""field_convert on the host backend (the plain loop of csrc/src/kernels/field_convert.hip) and
DistributedDomain.convert_from over several sub-domains. test_gpu_convert.py runs the same cases (convert_cases.py) on
the device."""
import pytest

import convert_cases as cases

PAIRS = pytest.mark.parametrize("pair", cases.PAIRS, ids=cases.pair_id)


@pytest.fixture
def host(st):
    return st.Backend.Host


@PAIRS
@pytest.mark.parametrize("size", cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bitwise_shapes(st, host, size, pair):
    cases.case_shape(st, host, size, pair)


@PAIRS
def test_curr_and_next_two_domains_and_one(st, host, pair):
    cases.case_buffers(st, host, pair)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@PAIRS
@pytest.mark.parametrize("name", sorted(cases.REGIONS))
def test_untouched_bytes(st, host, name, pair, stats):
    cases.case_region(st, host, name, pair, stats)


@PAIRS
@pytest.mark.parametrize("side", ["src", "dst"])
def test_unpadded_side(st, host, side, pair):
    cases.case_unpadded(st, host, side, pair)


@PAIRS
@pytest.mark.parametrize("name", ["align64", "align128", "shared_halo_line", "x_halo_align"])
def test_layouts(st, host, name, pair):
    cases.case_layout(st, host, name, pair)


@PAIRS
@pytest.mark.parametrize("axis", sorted(cases.CUTS))
def test_two_sub_domains(st, host, axis, pair):
    cases.case_cut(st, host, axis, pair)


@PAIRS
@pytest.mark.parametrize("size", [(10, 6, 4), (522, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_stats_exact(st, host, size, pair):
    cases.case_stats_exact(st, host, size, pair)


@PAIRS
@pytest.mark.parametrize("max_blocks", [1, 3])
def test_forced_grids(st, host, max_blocks, pair):
    cases.case_forced_grid(st, host, (24, 70, 6), pair, max_blocks)


@PAIRS
def test_stats_random_within_summation_bound(st, host, pair):
    cases.case_stats_random(st, host, pair)


@PAIRS
def test_stats_nonfinite(st, host, pair):
    cases.case_stats_nonfinite(st, host, pair)


@PAIRS
def test_stats_repeatable_bits(st, host, pair):
    cases.case_stats_repeatable(st, host, pair)


def test_launch_info(st, host):
    cases.case_launch_info(st, host)


def test_refusals(st, host):
    cases.case_refusals(st, host)


def test_exports(st):
    import stencil2_amd.ops as ops
    for name in ("field_convert", "field_convert_launch_info", "field_convert_supported", "convert_reference"):
        assert hasattr(ops, name), name
    for name in ("field_convert", "field_convert_launch_info", "field_convert_supported"):
        assert hasattr(st._C, name), name
    assert hasattr(st.DistributedDomain, "convert_from")
