"""Checks of k_nco_exact through nrsc5hip_stage_nco_exact, shared by tests/test_nco_exact_cpu.py (the CPU-emulated twin: the plain scalar form) and
tests/test_gpu_nco_exact.py (the gfx950 library: 64 lanes, a 512-byte table row per 64 steps, the 48-step tail of every symbol).  The expected table is
the float32 recurrence of tests/nco_args.py; everything is compared bit for bit."""
import numpy as np

from nrsc5_amd import engine as eng
from tests import nco_args as na

FILL = 0xA5A5A5A5


def make_engine(lib):
    return eng.Engine(max_streams=3, q15_capacity=2 * 71280, lib_path=lib)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def run_case(E, case):
    return E.stage_nco_exact(case["start"], case["inc"], case["active"], case["nco_mode"])


def check_case(E, k):
    """one launch of case k: the exact stream's table and end state, the other two streams' rows and states untouched; -> entries compared"""
    case = na.inputs()[k]
    tab, end = run_case(E, case)
    exp_tab, exp_end = na.expected()
    ex = case["exact"]
    got, want = _bits(tab[ex]), _bits(exp_tab[k])
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        for i in bad[:8]:
            print("%s: entry %d (symbol %d, step %d): got %08x %08x expected %08x %08x" % (case["name"], i, i // na.SYM_N, i % na.SYM_N, got[i, 0], got[i, 1], want[i, 0], want[i, 1]))
    assert bad.size == 0, "%s: %d of %d table entries differ, first at symbol %d step %d" % (case["name"], bad.size, want.shape[0], bad[0] // na.SYM_N, bad[0] % na.SYM_N)
    # named parts of the same comparison: the 48-step tail of every symbol and the renormalised first entry of every following one
    t = got.reshape(na.NSYM, na.SYM_N, 2); w = want.reshape(na.NSYM, na.SYM_N, 2)
    assert np.array_equal(t[:, 2112:], w[:, 2112:]) and np.array_equal(t[1:, 0], w[1:, 0])
    assert np.array_equal(_bits(end[ex]), _bits(exp_end[k])), "%s: oscillator after the block %r, expected %r" % (case["name"], end[ex], exp_end[k])
    for s in range(3):
        if s == ex:
            continue
        assert np.all(_bits(tab[s]) == FILL), "%s: stream %d (active %d, nco_mode %d) had table entries written" % (case["name"], s, case["active"][s], case["nco_mode"][s])
        assert np.array_equal(_bits(end[s]), _bits(case["start"][s])), "%s: stream %d's oscillator state changed" % (case["name"], s)
    return int(want.shape[0])
