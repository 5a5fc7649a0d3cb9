"""`-m "not gpu"`: reception steering (nrsc5hip_fm_steer*, k_fm_audio<true> in nrsc5_amd/csrc/k_fm_audio.hip) on the CPU-emulated twin against the
float64 restatement of its definition (tests/steer_model.py); the checks are tests/steer_checks.py, which tests/test_gpu_steer_stage.py runs on
gfx950.  The twin's "device" memory is host memory, so numpy buffers are passed by address here -- never to the real library."""
import pytest

from tests import fm_checks as fc, steer_args as sa, steer_checks as sc


@pytest.fixture(scope="module")
def be(emu_lib):
    return fc.Backend(emu_lib, gpu=False)


def test_inputs_hold_what_the_checks_take_for_granted():
    sa.analyse()


def test_factors_through_the_stage_hook(be):
    sc.check_factors(be)


@pytest.mark.parametrize("name", list(sa.CASES))
def test_audio_against_the_model_end_to_end_and_with_the_library_factors(be, name):
    sc.check_audio(be, name)


def test_exact_properties(be):
    sc.check_exact(be)


def test_narrow_table(be):
    sc.check_narrow_table(be)


def test_physical_condition(be):
    sc.check_physical(be)


@pytest.mark.parametrize("plan", list(fc.chunk_plans(sa.N)))
def test_chunking_is_bit_identical(be, plan):
    sc.check_chunking(be, [plan])


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_equal_their_single_channel_runs(be, k):
    sc.check_channels(be, k)


def test_life_cycle(be):
    sc.check_life_cycle(be)


def test_launch_counts(be):
    sc.check_launch_counts(be)
