"""GPU: the reception impairments (nrsc5hip_fm_impair*, nrsc5_amd/csrc/k_fm_impair.hip) on gfx950 against the float64 restatement of their
definition (tests/impair_model.py): the checks of tests/impair_checks.py, which tests/test_impair_stage_cpu.py runs on the CPU twin, with the
buffers on the device."""
import pytest

from tests import impair_checks as ic, fm_checks as fc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return fc.Backend(hip_lib, gpu=True)


def test_gpu_amplitude_band_pass_and_block_sums_through_the_stage_hook(be):
    ic.check_stage(be)


def test_gpu_the_stated_orders_hold_bit_for_bit(be):
    ic.check_orders(be)


def test_gpu_reports_figures_verdicts_and_clamps(be):
    ic.check_report(be)


def test_gpu_chunking_is_bit_identical(be):
    ic.check_chunking(be)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_equal_their_single_channel_runs(be, k):
    ic.check_channels(be, k)


def test_gpu_channel_7_of_9_equals_channel_0_of_1(be):
    ic.check_channel_7_of_9(be)


def test_gpu_life_cycle(be):
    ic.check_life_cycle(be)


def test_gpu_with_carrier_steering_rds_and_same_on(be):
    ic.check_with_everything_on(be)


@pytest.mark.parametrize("name", ["lr80", "fullscale", "cnr40"])
def test_gpu_audio_d_and_carrier_are_untouched_and_two_launches_are_added(be, name):
    ic.check_untouched(be, name)


def test_gpu_band_pass_taps_and_response(be):
    ic.check_taps(be)
