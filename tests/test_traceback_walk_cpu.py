"""CPU-emulator twin of tests/test_gpu_traceback_walk.py: the same device functions compiled for the SIMT emulator give the same bytes."""
import pytest

from tests import traceback_walk_checks as tw


@pytest.mark.parametrize("length", tw.LENGTHS + (tw.P1_LEN,))
def test_stage_walk_equals_block_and_oracle(emu_lib, oracle, length):
    tw.check_stage_lengths(emu_lib, oracle, length)


def test_engine_false_lock_records_identical(emu_lib):
    tw.check_engine_false_lock(emu_lib)
