"""GPU: coarse acquisition as the gfx950 code computes it, through the nrsc5hip_stage_acquire* hooks that run the production launches on caller
windows -- k_acq_list, k_acq_decimate, k_acq_fir, k_acq_corr, k_acq_peak on the FIFO and the zero-copy seam, the first section of k_am_block in its
256- and 512-lane forms -- against the oracle's twins on the inputs of tests/acq_args.py.  Every integer equal, every float equal in its bits, no
tolerance (tests/acq_checks.py); the same checks run on the emulated build in tests/test_acquire_stage_cpu.py, which also holds the tests of the
input sets themselves.  The shapes are the kernels' own fixed windows (71280 / 8910 samples); the list test is the only multi-stream one."""
import pytest

from tests import acq_args as aa, acq_checks as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fifo(hip_lib):
    e = ac.make_engine(hip_lib, "fifo", aa.LIST_N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def raw(hip_lib):
    e = ac.make_engine(hip_lib, "raw", 4)
    yield e
    e.close()


@pytest.fixture(scope="module", params=("am", "am-pipe"))
def am(hip_lib, request):
    e = ac.make_engine(hip_lib, request.param)
    yield e
    e.close()


@pytest.mark.parametrize("name", aa.single_names("fm"))
def test_gpu_fm_acquisition_equals_the_twins(fifo, oracle, name):
    ac.check_single(fifo, oracle, "fm", name)


def test_gpu_fm_acquisition_leaves_fine_and_short_streams_alone(fifo):
    ac.check_inactive(fifo, "fm")


def test_gpu_fm_acquisition_walks_a_list_of_65_active_streams(fifo, oracle):
    active, n = ac.check_list(fifo, oracle)
    assert active == 65 and n == 95


def test_gpu_fm_acquisition_decimates_its_window_at_rd(raw, oracle):
    ac.check_raw(raw, oracle)


@pytest.mark.parametrize("name", aa.single_names("am"))
def test_gpu_am_acquisition_equals_the_twins(am, oracle, name):
    ac.check_single(am, oracle, "am", name)


def test_gpu_am_acquisition_leaves_fine_and_short_streams_alone(am):
    ac.check_inactive(am, "am")


def test_gpu_fifo_hook_rejects_bad_arguments(fifo):
    ac.check_rejections_fifo(fifo)


def test_gpu_zero_copy_hook_rejects_bad_arguments(raw):
    ac.check_rejections_raw(raw)


def test_gpu_am_hook_rejects_bad_arguments(am):
    ac.check_rejections_am(am)
