"""`-m "not gpu"`: the reception impairments (nrsc5hip_fm_impair*, nrsc5_amd/csrc/k_fm_impair.hip) on the CPU-emulated twin against the float64
restatement of their definition (tests/impair_model.py); the checks are tests/impair_checks.py, which tests/test_gpu_impair_stage.py runs on
gfx950.  The twin's "device" memory is host memory, so numpy buffers are passed by address here -- never to the real library."""
import pytest

from nrsc5_amd import synth_fm as sf
from tests import fm_args as fa, fm_checks as fc, impair_args as ia, impair_checks as ic


@pytest.fixture(scope="module")
def be(emu_lib):
    return fc.Backend(emu_lib, gpu=False)


@pytest.mark.parametrize("name", list(ia.CASES))
def test_the_model_shows_what_the_input_is_named_for(name):
    ia.analyse(name)


def test_rays_are_refused_with_rds_or_same():
    with pytest.raises(ValueError):
        sf.fm_host(1000, rays=[(0.3, 5e-6, 2.0)], rds=dict(groups=sf.rds_groups(0x1234)))
    with pytest.raises(ValueError):
        sf.fm_carrier(1000, rays=[(0.3, 5e-6, 2.0)], same=dict(bursts=[(0.0, "ZCZC-")]))
    assert sf.fm_carrier(1000, rays=[]).shape == (1000,)


def test_amplitude_band_pass_and_block_sums_through_the_stage_hook(be):
    ic.check_stage(be)


def test_the_stated_orders_hold_bit_for_bit(be):
    ic.check_orders(be)


def test_reports_figures_verdicts_and_clamps(be):
    ic.check_report(be)


@pytest.mark.parametrize("plan", list(ic.chunk_plans(ia.N)))
def test_chunking_is_bit_identical(be, plan):
    ic.check_chunking(be, [plan])


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_equal_their_single_channel_runs(be, k):
    ic.check_channels(be, k)


def test_channel_7_of_9_equals_channel_0_of_1(be):
    ic.check_channel_7_of_9(be)


def test_life_cycle(be):
    ic.check_life_cycle(be)


def test_with_carrier_steering_rds_and_same_on(be):
    ic.check_with_everything_on(be)


@pytest.mark.parametrize("name", ["lr80", "fullscale", "cnr40"])
def test_audio_d_and_carrier_are_untouched_and_two_launches_are_added(be, name):
    ic.check_untouched(be, name)


def test_band_pass_taps_and_response(be):
    ic.check_taps(be)
