"""Pinned plans on the device backend with every sub-domain on device 0: plan_summary() byte for byte against the
fixtures of tests/golden/plans/ (recorded on an MI355X by plan_cases.py --gpu). Every case first runs one exchange
against the coordinate oracle, so the pinned plan is a working one and realize()'s buffers, IPC handshake and
segment lists have run. test_plan_pinned.py pins the host backend's plans."""
import pytest

import plan_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(cases.GPU_SINGLE))
def test_single_process_plan(st, name):
    cases.check_single(name, cases.gpu_single_summary(st, name))


@pytest.mark.parametrize("name", sorted(cases.GPU_RANKS))
def test_two_ranks_one_gpu_plan(name):
    cases.check_ranks(name, cases.gpu_rank_summaries(name))
