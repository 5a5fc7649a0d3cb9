"""GPU: SAME on the analog FM object (nrsc5hip_fm_same_*, nrsc5_amd/csrc/k_same.hip) on gfx950 against the float64 restatement of its definition
(tests/same_model.py): the checks of tests/same_checks.py, which tests/test_same_stage_cpu.py runs on the CPU twin, with the buffers on the device."""
import pytest

from tests import same_args as sa, same_checks as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return sc.Backend(hip_lib, gpu=True)


def test_gpu_table_grid_and_latency(be):
    sc.check_table(be)


def test_gpu_tone_sums_timing_and_bits_through_the_stage_hook(be):
    sc.check_stage_signal(be)


@pytest.mark.parametrize("name", list(sa.CASES))
def test_gpu_session_equals_model(be, name):
    sc.check_session_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_with_different_schedules(be, k):
    sc.check_multi(be, k)


@pytest.mark.parametrize("plan", list(sc.chunk_plans()))
def test_gpu_chunking_gives_identical_events(be, plan):
    sc.check_chunking(be, [plan])


def test_gpu_reset_and_enable_rules(be):
    sc.check_reset_and_enable(be)


def test_gpu_audio_and_d_are_untouched(be):
    sc.check_audio_untouched(be)


def test_gpu_launch_counts_without_and_with_same(be):
    sc.check_launch_counts(be)


@pytest.mark.parametrize("name", list(sa.frame_cases()))
def test_gpu_frames_equal_model(be, name):
    sc.check_frames_case(be, name)


def test_gpu_frames_stream_continues_in_the_next_call(be):
    sc.check_frames_in_pieces(be)


def test_gpu_frames_of_several_channels(be):
    sc.check_frames_many_channels(be)
