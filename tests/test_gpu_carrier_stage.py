"""GPU: the carrier measurement (nrsc5hip_fm_carrier*, nrsc5_amd/csrc/k_fm_carrier.hip) on gfx950 against the float64 restatement of its
definition (tests/carrier_model.py): the checks of tests/carrier_checks.py, which tests/test_carrier_stage_cpu.py runs on the CPU twin, with
the buffers on the device."""
import pytest

from tests import carrier_checks as cc, fm_args as fa, fm_checks as fc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return fc.Backend(hip_lib, gpu=True)


def test_gpu_envelope_and_block_sums_through_the_stage_hook(be):
    cc.check_stage_sums(be)


def test_gpu_reports_are_the_stated_sums_and_the_clamps_hold(be):
    cc.check_report(be)


def test_gpu_physical_condition(be):
    cc.check_physical(be)


def test_gpu_chunking_is_bit_identical(be):
    cc.check_chunking(be)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_equal_their_single_channel_runs(be, k):
    cc.check_channels(be, k)


def test_gpu_life_cycle(be):
    cc.check_life_cycle(be)


@pytest.mark.parametrize("name", list(fa.CASES))
def test_gpu_audio_and_d_are_untouched(be, name):
    cc.check_untouched_audio(be, name)
