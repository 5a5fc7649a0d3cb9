"""`-m "not gpu"`: the analog FM demodulator (nrsc5hip_fm_*, nrsc5_amd/csrc/k_fm_audio.hip) on the CPU-emulated twin against the float64
restatement of its definition (tests/fm_model.py); the checks are tests/fm_checks.py, which tests/test_gpu_fm_stage.py runs on gfx950.  The
twin's "device" memory is host memory, so numpy buffers are passed by address here -- never to the real library."""
import pytest

from tests import fm_args as fa, fm_checks as fc


@pytest.fixture(scope="module")
def be(emu_lib):
    return fc.Backend(emu_lib, gpu=False)


def test_filter_responses(be):
    fc.check_filter_responses(be)


@pytest.mark.parametrize("name", list(fa.CASES))
def test_audio_equals_float64_model(be, name):
    fc.check_audio_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_with_different_programmes(be, k):
    fc.check_audio_multi(be, k)


def test_discriminator_and_block_sums_through_the_stage_hook(be):
    fc.check_stage_d(be)


@pytest.mark.parametrize("plan", list(fc.chunk_plans(fa.N)))
def test_chunking_is_byte_identical(be, plan):
    fc.check_chunking(be, [plan])


def test_reset_overflow_and_rejected_arguments(be):
    fc.check_reset_overflow_bad_arguments(be)


def test_edge_cases(be):
    fc.check_edges(be)


def test_physical_checks(be):
    fc.check_physical(be)
