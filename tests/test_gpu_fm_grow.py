"""GPU: the analog FM object's buffers that grow (nrsc5_amd/csrc/fm_host.h) on gfx950: the checks of tests/fm_grow_checks.py, which
tests/test_fm_grow_cpu.py runs on the CPU twin, with the buffers on the device."""
import pytest

from tests import fm_checks as fc, fm_grow_checks as gc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return fc.Backend(hip_lib, gpu=True)


def test_gpu_one_push_that_grows_every_array_equals_the_chunked_run(be):
    gc.check_arrays_grow(be)


def test_gpu_one_push_that_grows_both_event_arenas_equals_the_chunked_run(be):
    gc.check_arenas_grow(be)
