"""GPU: k_nco_exact as the gfx950 code runs it (nrsc5hip_stage_nco_exact) -- all 64 lanes of a wave on the same recurrence, lane j & 63 holding step j's
phasor, one 512-byte table row per 64 steps and a 48-step tail per symbol -- against the float32 recurrence of tests/nco_args.py, bit for bit, under
the checks of tests/nco_checks.py: every table entry, the oscillator state after the block, and the rows of the streams the kernel must leave alone."""
import pytest

from tests import nco_args as na, nco_checks as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = nc.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("k", range(len(na.CASES)), ids=[c[0] for c in na.CASES])
def test_gpu_table_and_state_equal_the_float_recurrence(E, k):
    assert nc.check_case(E, k) == 32 * 2160
