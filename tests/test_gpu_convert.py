"""field_convert on the device (csrc/src/kernels/field_convert.hip: the row kernel of the aligned vector layout and
the one-thread-per-cell kernel) and DistributedDomain.convert_from over several sub-domains per GPU. test_convert.py
runs the same cases (convert_cases.py) on the host backend."""
import pytest

import convert_cases as cases

pytestmark = pytest.mark.gpu

PAIRS = pytest.mark.parametrize("pair", cases.PAIRS, ids=cases.pair_id)


@pytest.fixture
def dev(st):
    return st.Backend.Device


@PAIRS
@pytest.mark.parametrize("size", cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bitwise_shapes(st, dev, size, pair):
    cases.case_shape(st, dev, size, pair)


@PAIRS
def test_curr_and_next_two_domains_and_one(st, dev, pair):
    cases.case_buffers(st, dev, pair)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@PAIRS
@pytest.mark.parametrize("name", sorted(cases.REGIONS))
def test_untouched_bytes(st, dev, name, pair, stats):
    cases.case_region(st, dev, name, pair, stats)


@PAIRS
@pytest.mark.parametrize("side", ["src", "dst"])
def test_unpadded_side(st, dev, side, pair):
    cases.case_unpadded(st, dev, side, pair)


@PAIRS
@pytest.mark.parametrize("name", ["align64", "align128", "shared_halo_line", "x_halo_align"])
def test_layouts(st, dev, name, pair):
    cases.case_layout(st, dev, name, pair)


@PAIRS
@pytest.mark.parametrize("axis", sorted(cases.CUTS))
def test_two_sub_domains(st, dev, axis, pair):
    cases.case_cut(st, dev, axis, pair)


@PAIRS
@pytest.mark.parametrize("size", [(10, 6, 4), (522, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_stats_exact(st, dev, size, pair):
    cases.case_stats_exact(st, dev, size, pair)


@PAIRS
@pytest.mark.parametrize("max_blocks", [1, 3])
def test_forced_grids(st, dev, max_blocks, pair):
    cases.case_forced_grid(st, dev, (24, 70, 6), pair, max_blocks)


@PAIRS
def test_stats_random_within_summation_bound(st, dev, pair):
    cases.case_stats_random(st, dev, pair)


@PAIRS
def test_stats_nonfinite(st, dev, pair):
    cases.case_stats_nonfinite(st, dev, pair)


@PAIRS
def test_stats_repeatable_bits(st, dev, pair):
    cases.case_stats_repeatable(st, dev, pair)


def test_launch_info(st, dev):
    cases.case_launch_info(st, dev)


def test_refusals(st, dev):
    cases.case_refusals(st, dev)
