"""GPU: the analog FM demodulator (nrsc5hip_fm_*, nrsc5_amd/csrc/k_fm_audio.hip) on gfx950 against the float64 restatement of its definition
(tests/fm_model.py): the checks of tests/fm_checks.py, which tests/test_fm_stage_cpu.py runs on the CPU twin, with the buffers on the device."""
import pytest

from tests import fm_args as fa, fm_checks as fc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return fc.Backend(hip_lib, gpu=True)


def test_gpu_filter_responses(be):
    fc.check_filter_responses(be)


@pytest.mark.parametrize("name", list(fa.CASES))
def test_gpu_audio_equals_float64_model(be, name):
    fc.check_audio_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_gpu_channels_with_different_programmes(be, k):
    fc.check_audio_multi(be, k)


def test_gpu_discriminator_and_block_sums_through_the_stage_hook(be):
    fc.check_stage_d(be)


def test_gpu_chunking_is_byte_identical(be):
    fc.check_chunking(be)


def test_gpu_reset_overflow_and_rejected_arguments(be):
    fc.check_reset_overflow_bad_arguments(be)


def test_gpu_edge_cases(be):
    fc.check_edges(be)


def test_gpu_physical_checks(be):
    fc.check_physical(be)
