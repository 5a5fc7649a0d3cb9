"""`-m "not gpu"`: the analog FM object's buffers that grow (nrsc5_amd/csrc/fm_host.h) on the CPU-emulated twin; the checks are
tests/fm_grow_checks.py, which tests/test_gpu_fm_grow.py runs on gfx950."""
import pytest

from tests import fm_checks as fc, fm_grow_checks as gc


@pytest.fixture(scope="module")
def be(emu_lib):
    return fc.Backend(emu_lib, gpu=False)


def test_one_push_that_grows_every_array_equals_the_chunked_run(be):
    gc.check_arrays_grow(be)


def test_one_push_that_grows_both_event_arenas_equals_the_chunked_run(be):
    gc.check_arenas_grow(be)
