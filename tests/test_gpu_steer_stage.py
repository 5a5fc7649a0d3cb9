"""GPU: reception steering (nrsc5hip_fm_steer*, k_fm_audio<true> in nrsc5_amd/csrc/k_fm_audio.hip) on gfx950 against the float64 restatement of its
definition (tests/steer_model.py): the checks of tests/steer_checks.py, which tests/test_steer_stage_cpu.py runs on the CPU twin, with the
buffers on the device."""
import pytest

from tests import fm_checks as fc, steer_args as sa, steer_checks as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return fc.Backend(hip_lib, gpu=True)


def test_gpu_factors_through_the_stage_hook(be):
    sc.check_factors(be)


@pytest.mark.parametrize("name", list(sa.CASES))
def test_gpu_audio_against_the_model_end_to_end_and_with_the_library_factors(be, name):
    sc.check_audio(be, name)


def test_gpu_exact_properties(be):
    sc.check_exact(be)


def test_gpu_narrow_table(be):
    sc.check_narrow_table(be)


def test_gpu_physical_condition(be):
    sc.check_physical(be)


def test_gpu_chunking_is_bit_identical(be):
    sc.check_chunking(be)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_equal_their_single_channel_runs(be, k):
    sc.check_channels(be, k)


def test_gpu_life_cycle(be):
    sc.check_life_cycle(be)


def test_gpu_launch_counts(be):
    sc.check_launch_counts(be)
