"""Pinned plans on the host backend: plan_summary() of one process with 1, 2 and 4 sub-domains (methods, radii and
a non-periodic x axis) and of 2, 3 and 4 ranks of the TCP group (one host, and 4 ranks as two nodes of two), byte for
byte against the fixtures of tests/golden/plans/ (plan_cases.py records them). test_gpu_plan_pinned.py pins the
device backend's plans the same way."""
import pytest

import plan_cases as cases


@pytest.mark.parametrize("name", sorted(cases.SINGLE))
def test_single_process_plan(st, name):
    cases.check_single(name, cases.single_summary(st, name))


def test_plan_repeats_in_one_process(st):
    name = "four-all-fec"
    assert cases.single_summary(st, name) == cases.single_summary(st, name)


@pytest.mark.parametrize("name", sorted(cases.RANKS))
def test_ranks_plan(name):
    cases.check_ranks(name, cases.host_rank_summaries(name))
