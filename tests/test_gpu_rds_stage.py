"""GPU: RDS on the analog FM object (nrsc5hip_fm_rds_*, nrsc5_amd/csrc/k_rds.hip) on gfx950 against the float64 restatement of its definition
(tests/rds_model.py): the checks of tests/rds_checks.py, which tests/test_rds_stage_cpu.py runs on the CPU twin, with the buffers on the device."""
import pytest

from tests import rds_args as ra, rds_checks as rc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return rc.Backend(hip_lib, gpu=True)


def test_gpu_tables(be):
    rc.check_tables(be)


def test_gpu_matched_filter_timing_and_bits_through_the_stage_hook(be):
    rc.check_stage_signal(be)


@pytest.mark.parametrize("name", list(ra.CASES))
def test_gpu_session_equals_model(be, name):
    rc.check_session_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_with_different_schedules(be, k):
    rc.check_multi(be, k)


@pytest.mark.parametrize("plan", list(rc.chunk_plans(ra.N)))
def test_gpu_chunking_gives_identical_events(be, plan):
    rc.check_chunking(be, [plan])


def test_gpu_reset_and_enable_rules(be):
    rc.check_reset_and_enable(be)


def test_gpu_audio_is_untouched(be):
    rc.check_audio_untouched(be)


def test_gpu_launch_counts_without_and_with_rds(be):
    rc.check_launch_counts(be)


@pytest.mark.parametrize("name", list(ra.group_cases()))
def test_gpu_groups_equal_model(be, name):
    rc.check_groups_case(be, name)


def test_gpu_groups_stream_continues_in_the_next_call(be):
    rc.check_groups_in_pieces(be)


def test_gpu_groups_of_several_channels(be):
    rc.check_groups_many_channels(be)
