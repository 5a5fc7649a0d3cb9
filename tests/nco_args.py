"""Cases for the checks of k_nco_exact (tests/nco_checks.py), written once: the oscillator states a block starts from and the float32 recurrence of the
reference (acquire.c:237-252) restated in numpy as the expected table.

Every case is one launch on three streams -- one active in exact mode, one inactive, one active on the closed form (nco_mode = 0) -- with the roles on
different stream indices from case to case.  The exact stream's phase_increment is the float pair (cos, sin) of the per-sample rotation of a carrier
offset of 0, +300 and -300 Hz at 744 187.5 S/s; one case starts from a phasor of magnitude 1.25, which the first renormalisation has to bring back."""
import functools

import numpy as np

NSYM, SYM_N = 32, 2160
FS = 744187.5
F32 = np.float32

# name, carrier offset (Hz), start angle (rad), start magnitude, (exact, inactive, closed-form) stream index
CASES = (("cfo 0", 0.0, 0.7, 1.0, (0, 1, 2)),
         ("cfo +300", 300.0, -2.1, 1.0, (1, 2, 0)),
         ("cfo -300", -300.0, 3.0, 1.0, (2, 0, 1)),
         ("cfo +300, |start| 1.25", 300.0, 0.3, 1.25, (0, 2, 1)))


def _pair(angle, mag=1.0):
    return np.array([F32(mag) * F32(np.cos(angle)), F32(mag) * F32(np.sin(angle))], dtype=F32)


@functools.lru_cache(maxsize=None)
def inputs():
    """-> per case dict(start [3, 2], inc [3, 2], active [3], nco_mode [3], exact = index of the exact stream); read-only"""
    out = []
    for k, (name, cfo, a0, mag, (ex, off, closed)) in enumerate(CASES):
        start, inc = np.zeros((3, 2), dtype=F32), np.zeros((3, 2), dtype=F32)
        active, mode = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
        step = -2.0 * np.pi * cfo / FS
        # the streams the kernel must leave alone get a state it could run on all the same
        for s, (act, md) in ((ex, (1, 1)), (off, (0, 1)), (closed, (1, 0))):
            start[s] = _pair(a0 + 0.1 * s, mag); inc[s] = _pair(step); active[s] = act; mode[s] = md
        for v in (start, inc, active, mode):
            v.setflags(write=False)
        out.append(dict(name=name, start=start, inc=inc, active=active, nco_mode=mode, exact=ex))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected():
    """-> (tab float32 [cases, 32 * 2160, 2], end float32 [cases, 2]) of the exact stream of every case: phase *= phase_increment as the four float
    products and two float sums it is, 2160 times per symbol, then phase /= cabsf(phase) with cabsf = sqrt of the double sum rounded once to float
    (glibc's hypotf) and two float divisions.  All cases advance together, one numpy operation per float operation."""
    ins = inputs()
    pr = np.array([c["start"][c["exact"], 0] for c in ins], dtype=F32)
    pi = np.array([c["start"][c["exact"], 1] for c in ins], dtype=F32)
    c = np.array([x["inc"][x["exact"], 0] for x in ins], dtype=F32)
    d = np.array([x["inc"][x["exact"], 1] for x in ins], dtype=F32)
    tab = np.zeros((len(ins), NSYM * SYM_N, 2), dtype=F32)
    for sym in range(NSYM):
        for j in range(SYM_N):
            tab[:, sym * SYM_N + j, 0] = pr; tab[:, sym * SYM_N + j, 1] = pi
            ac, bd, ad, bc = pr * c, pi * d, pr * d, pi * c
            pr, pi = ac - bd, ad + bc
            assert pr.dtype == F32 and pi.dtype == F32
        m = np.sqrt(pr.astype(np.float64) * pr.astype(np.float64) + pi.astype(np.float64) * pi.astype(np.float64)).astype(F32)
        pr, pi = pr / m, pi / m
    end = np.stack([pr, pi], axis=1).astype(F32)
    tab.setflags(write=False); end.setflags(write=False)
    return tab, end
