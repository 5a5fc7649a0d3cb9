"""`-m "not gpu"`: the carrier measurement (nrsc5hip_fm_carrier*, nrsc5_amd/csrc/k_fm_carrier.hip) on the CPU-emulated twin against the float64
restatement of its definition (tests/carrier_model.py); the checks are tests/carrier_checks.py, which tests/test_gpu_carrier_stage.py runs on
gfx950.  The twin's "device" memory is host memory, so numpy buffers are passed by address here -- never to the real library."""
import pytest

from tests import carrier_args as ca, carrier_checks as cc, fm_args as fa, fm_checks as fc


@pytest.fixture(scope="module")
def be(emu_lib):
    return fc.Backend(emu_lib, gpu=False)


def test_envelope_and_block_sums_through_the_stage_hook(be):
    cc.check_stage_sums(be)


def test_reports_are_the_stated_sums_and_the_clamps_hold(be):
    cc.check_report(be)


def test_physical_condition(be):
    cc.check_physical(be)


@pytest.mark.parametrize("plan", list(fc.chunk_plans(ca.N)))
def test_chunking_is_bit_identical(be, plan):
    cc.check_chunking(be, [plan])


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_equal_their_single_channel_runs(be, k):
    cc.check_channels(be, k)


def test_life_cycle(be):
    cc.check_life_cycle(be)


@pytest.mark.parametrize("name", list(fa.CASES))
def test_audio_and_d_are_untouched(be, name):
    cc.check_untouched_audio(be, name)
