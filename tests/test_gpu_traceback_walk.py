"""Single-path P1 traceback on the device: the walk (16-byte staging, per-lane bit-parallel re-encode count) + check against the
block-parallel traceback and the oracle's decoder."""
import pytest

from tests import traceback_walk_checks as tw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", tw.LENGTHS + (tw.P1_LEN,))
def test_stage_walk_equals_block_and_oracle(hip_lib, oracle, length):
    tw.check_stage_lengths(hip_lib, oracle, length)


def test_engine_false_lock_records_identical(hip_lib):
    tw.check_engine_false_lock(hip_lib)
