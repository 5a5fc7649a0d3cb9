"""`-m "not gpu"`: k_nco_exact on the CPU-emulated twin (the plain scalar form of the recurrence) through nrsc5hip_stage_nco_exact -- the hook itself
and the checks of tests/nco_checks.py on the cases of tests/nco_args.py.  The same checks run on the gfx950 code in tests/test_gpu_nco_exact.py."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import nco_args as na, nco_checks as nc


@pytest.fixture(scope="module")
def E(emu_lib):
    e = nc.make_engine(emu_lib)
    yield e
    e.close()


@pytest.mark.parametrize("k", range(len(na.CASES)), ids=[c[0] for c in na.CASES])
def test_table_and_state_equal_the_float_recurrence_on_the_emulated_build(E, k):
    assert nc.check_case(E, k) == 32 * 2160


def test_cases_hold_what_they_are_meant_to_hold():
    ins = na.inputs()
    assert sorted(c["exact"] for c in ins[:3]) == [0, 1, 2]                      # the exact stream sits on every index once
    for c in ins:
        ex = c["exact"]
        assert c["active"][ex] == 1 and c["nco_mode"][ex] == 1 and sorted(zip(c["active"].tolist(), c["nco_mode"].tolist())) == [(0, 1), (1, 0), (1, 1)]
    mags = [float(np.hypot(*c["start"][c["exact"]].astype(np.float64))) for c in ins]
    assert all(abs(m - 1.0) < 1e-6 for m in mags[:3]) and abs(mags[3] - 1.25) < 1e-6
    assert ins[0]["inc"][ins[0]["exact"]].tolist() == [1.0, 0.0] and ins[1]["inc"][ins[1]["exact"], 1] < 0 < ins[2]["inc"][ins[2]["exact"], 1]
    tab, end = na.expected()
    # the recurrence does something: the phasor turns, and the first renormalisation brings the 1.25 back
    assert not np.array_equal(tab[1, 0], tab[1, 2159]) and abs(float(np.hypot(*tab[3, 2160].astype(np.float64))) - 1.0) < 1e-6 < abs(float(np.hypot(*tab[3, 2159].astype(np.float64))) - 1.0)


def test_stage_nco_exact_rejects_bad_arguments(E):
    c = na.inputs()[0]
    with pytest.raises(eng.Nrsc5HipError) as ei:
        E.stage_nco_exact(c["start"], c["inc"], c["active"], None, n=3)
    assert ("error %d:" % eng.EINVAL) in str(ei.value)
    for n in (0, 4):
        with pytest.raises((eng.Nrsc5HipError, ValueError)):
            E.stage_nco_exact(np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), n=n)
