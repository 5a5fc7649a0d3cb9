"""Inputs and tolerances for the checks of the FM symbol transform (tests/sym_checks.py), written once, fixed seeds.  One hook call is one block of 32 symbols -- the
kernel's own unit -- on 1 to 3 streams of an engine with max_streams = 4; a CALL below is the list of its streams' cases (and the launch's stream list).

THE CASES (amplitudes: a group at ~20 LSB rms, a group at full scale: +-32767 in the FIFO, bytes 0 and 255 in a capture)
  tones      every symbol a complex exponential at one FFT bin, pulse-shaped as the transmitter shapes it (sample j times shape[j]: the fold then adds sin^2 + cos^2 = 1
             and the tone falls on ONE bin).  Bins after the mix: the live edges and both sides of them (477, 478, 744, 745, 1303, 1304, 1570, 1571), DC (1024) and
             interior bins of both sidebands.  Once directly (dtheta = 0) and once k bins away with dtheta = 2 pi k / 2048, k = +-1, +-38, +-80, so that the mix has to
             move it.  The 20 LSB cases carry in-band bins only: a tone of amplitude 20 peaks at 20 * 2048 / 32767 = 1.25 while the rounding of its samples to integers
             alone leaves ~0.002 in every bin, more than the 1e-3 of the peak a dropped tone may leave.
  impulses   one non-zero sample at j = 0, 1, 111, 112, 2047, 2048, 2159 of the symbols 0, 1, 15, 16, 31, every other sample zero: seven cases, so that every one of the
             five symbols meets every j.  A symbol without an impulse must come out as exact zeros (its bound is zero).
  noise      full-band complex Gaussian, every symbol different; as a FIFO window at 20 LSB rms and at 9000 LSB rms clipped to +-32767, as a capture of uniform
             bytes, of bytes 0 / 255 only, and of bytes 126 .. 128
  phase      theta 0, +-pi, 3.0, -3.1; dtheta 0, 1e-9, +-0.2449, 2 pi 37.3 / 2048; growth 0, +-6e-8, +-1e-6 (the last not a value the receiver produces: it makes a
             missing or mis-scaled nco_ramp a 2e-3 effect)
  position   captures at a00 = 0, 3, 6, 7, 8, 9, 10, 2160 * 5 + 1 (the dword path of a0 < 7, the first vector-loaded start, every dword phase), every lead;
             FIFO windows at a00 = 0, 1, 1080
  exact      nco_mode = 1 on two tables: the float32 recurrence of tests/nco_args.py (what production holds) and arbitrary phasors of magnitude 0.9 .. 1.1 that
             differ per sample and per symbol
  inactive   three streams, the middle one with active = 0
  multi      a capture, a FIFO window and an exact-mode stream in one launch, without a stream list and with the list (2, 0, 1)
  prepare    (params_mode 1) FINE states: samperr +-10, cfo 0 and +-3, angle and prev_angle non-zero
  rawfifo    a capture and the FIFO window that holds its integer half-band, same parameters, side by side

THE TOLERANCE of a bin of symbol s (nothing here is measured on the kernel under test, nor on its emulated twin):
  4 x SYM_ERR_MEASURED x max |model bin of symbol s|  +  (closed-form cases only)  P_ERR x sum_j shape[j] |sample_j| / 32767
  SYM_ERR_MEASURED  tests/sym_model.py's reference32 -- the reference's float32 arithmetic, unfused, with the oracle's FFT, on the model's phasors rounded to float32 --
                    against the float64 model over every case below: the largest error of a bin relative to its symbol's largest live bin.  Measured 3.53e-7 (an
                    impulse case: every bin is as large as the largest; noise inputs 2.1e-7, tones 1.7e-7).  A symbol whose tone the cut drops has no live bin to
                    speak of -- the largest is 1e-7 of the tone the arithmetic is busy with -- and is measured against its case's in-band peak (7e-8).
                    tests/test_symbol_stage_cpu.py asserts that the reference arithmetic stays within it.  The device gets 4 x that, as the AM block-step test gives
                    it: it runs another, equally valid float32 factorisation (8 x 16 x 16 or 8 x 8 x 8 x 4, twiddles from a table, scale carried by the phasor).
  P_ERR             the closed-form phasor's worst absolute error, derived: csrc/fastmath.h states |error| <= 5e-7 for the sine and cosine of fast_sincos_reduced
                    (tests/math_checks.py holds the device to it: SIN_COS_HEADER), and between that evaluation and the sample the phasor passes through at most 17
                    complex products (16 steps of the recurrence ph *= stp, one with the sample), each a float32 complex product whose error is at most 3 x 2^-24 of
                    its magnitude (two products and a sum per component): 5e-7 + 17 * 3 * 2^-24 = 3.54e-6.  An error e of every phasor moves a bin by at most
                    e x sum_j shape[j] |sample_j| / 32767.
  Every case's bound stays below 1e-4 of its symbol's largest bin (asserted by the CPU test); the golden end-to-end runs hold the same floats to 1e-4 after
  equalisation."""
import functools

import numpy as np

from tests import halfband_args as ha, nco_args as na, sym_model as M

SYM_ERR_MEASURED = 3.6e-7                  # measured 3.53e-7 (see above), rounded up
SYM_FACTOR = 4.0
P_ERR = 5e-7 + 17 * 3 * 2.0 ** -24         # 3.54e-6
RMS_LSB = 20.0
FORMS = (1, 2, 4, 8, 16, 32)
MAX_STREAMS = 4
BLOCK = M.NSYM * M.SYM_N
EDGE_BINS = (477, 478, 744, 745, 1303, 1304, 1570, 1571)
BINS_ALL = EDGE_BINS + (1024, 500, 611, 700, 1400, 1450, 1555)
BINS_IN = tuple(b for b in BINS_ALL if M.slot_of(b) >= 0)
SHIFTS = (1, -1, 38, -38, 80, -80)
IMPULSE_J = (0, 1, 111, 112, 2047, 2048, 2159)
IMPULSE_SYMS = (0, 1, 15, 16, 31)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import port
    return port.Oracle()


def _ro(a):
    a.setflags(write=False)
    return a


def _case(name, kind, samples, **kw):
    c = dict(name=name, kind=kind, samples=_ro(samples), a00=0, lead=0, theta=0.0, dtheta=0.0, growth=0.0, active=1, tab=None, tone_bins=None)
    c.update(kw)
    return c


def _gauss(seed, rms, n=BLOCK):
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, rms / np.sqrt(2.0), size=(n, 2))
    return np.clip(np.rint(v), -32767, 32767).astype(np.int16)


def _tone_case(name, amp, bins, k, seed, **kw):
    """symbol i: amp * shape[j] * exp(2 pi i f j / 2048 + i phi_i) at bin bins[i % len] - k IN FRONT of the mix, stored conjugated as Q15 integers"""
    rng = np.random.default_rng(seed)
    sh, j = M.shape64(), np.arange(M.SYM_N)
    q = np.zeros((M.NSYM, M.SYM_N, 2), dtype=np.int16)
    after = [bins[i % len(bins)] for i in range(M.NSYM)]
    for i, b in enumerate(after):
        x = amp * sh * np.exp(1j * (2 * np.pi * (b - k - 1024) * j / M.FFT_N + rng.uniform(-np.pi, np.pi)))
        q[i, :, 0], q[i, :, 1] = np.rint(x.real), np.rint(-x.imag)
    return _case(name, "fifo", q.reshape(-1, 2), dtheta=2 * np.pi * k / M.FFT_N, tone_bins=tuple(after), amp=amp, **kw)


def _impulse_case(r):
    q = np.zeros((M.NSYM, M.SYM_N, 2), dtype=np.int16)
    values = ((32767, -12345), (-32767, 32767), (20, -7), (-3, 19), (12000, 32767))
    for i, sym in enumerate(IMPULSE_SYMS):
        q[sym, IMPULSE_J[(i + r) % 7]] = values[(i + r) % 5]
    return _case("impulse %d" % r, "fifo", q.reshape(-1, 2), theta=0.4 * r - 1.0, dtheta=(0.0, 0.0131, -0.2449)[r % 3], growth=(0.0, 6e-8)[r % 2])


def _capture(name, dwords):
    rng = np.random.default_rng(5200 + len(name))
    if name == "uniform":
        return rng.integers(0, 256, size=4 * dwords, dtype=np.uint8)
    if name == "fullscale":
        return rng.choice(np.array([0, 255], dtype=np.uint8), size=4 * dwords)
    return rng.integers(126, 129, size=4 * dwords, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def tables():
    """the two oscillator tables float32 [32, 2160, 2]: the reference's recurrence (carrier +300 Hz, tests/nco_args.py case 1), and arbitrary phasors"""
    rec = np.array(na.expected()[0][1], dtype=np.float32).reshape(M.NSYM, M.SYM_N, 2)
    rng = np.random.default_rng(77)
    ang, mag = rng.uniform(-np.pi, np.pi, size=(M.NSYM, M.SYM_N)), rng.uniform(0.9, 1.1, size=(M.NSYM, M.SYM_N))
    arb = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1).astype(np.float32)
    return _ro(rec), _ro(arb)


@functools.lru_cache(maxsize=None)
def calls():
    """-> {call name: dict(cases = the streams' cases, ids = None or the launch's stream list)}; read-only"""
    out = {}

    def add(name, cases, ids=None):
        assert 1 <= len(cases) <= 3 and name not in out
        out[name] = dict(name=name, cases=tuple(cases), ids=ids)

    # tones
    full = [_tone_case("tone direct full", 32767.0, BINS_ALL, 0, 100, theta=0.3)]
    low = [_tone_case("tone direct low", RMS_LSB, BINS_IN, 0, 101, theta=-2.0)]
    for n, k in enumerate(SHIFTS):
        if n % 2 == 0:
            full.append(_tone_case("tone shift %+d full" % k, 32767.0, BINS_ALL, k, 110 + n, theta=0.5 * n))
        else:
            low.append(_tone_case("tone shift %+d low" % k, RMS_LSB, BINS_IN, k, 110 + n, theta=-0.5 * n))
    add("tones a", full[:3]); add("tones b", [full[3]] + low[:2]); add("tones c", low[2:])
    # impulses
    imp = [_impulse_case(r) for r in range(7)]
    add("impulses a", imp[:3]); add("impulses b", imp[3:6]); add("impulses c", imp[6:])
    # noise
    uni, fs, near = _capture("uniform", BLOCK + 16), _capture("fullscale", BLOCK + 16), _capture("near", BLOCK + 16)
    add("noise fifo", [_case("noise fifo low", "fifo", _gauss(1, RMS_LSB)), _case("noise fifo full", "fifo", _gauss(2, 9000.0))])
    add("noise raw", [_case("noise raw uniform", "raw", uni, a00=16, lead=4), _case("noise raw 0/255", "raw", fs, a00=13, lead=8), _case("noise raw 126..128", "raw", near, a00=11, lead=12)])
    # phase
    ph = [(np.pi, 1e-9, 6e-8), (-np.pi, 0.2449, -6e-8), (3.0, -0.2449, 1e-6), (-3.1, 2 * np.pi * 37.3 / M.FFT_N, -1e-6), (0.0, 0.0, 1e-6), (0.0, 0.05, -6e-8)]
    pc = [_case("phase theta %.4g dtheta %.4g growth %.1g" % p, "fifo", _gauss(20 + i, (RMS_LSB, 9000.0)[i % 2]), theta=p[0], dtheta=p[1], growth=p[2]) for i, p in enumerate(ph)]
    add("phase a", pc[:3]); add("phase b", pc[3:])
    # position
    big = _capture("uniform", M.SYM_N * 5 + 1 + BLOCK + 5)
    pos = [_case("raw a00 %d lead %d" % (a, ha.LEADS[i % 4]), "raw", big, a00=a, lead=ha.LEADS[i % 4], theta=0.1 * i, dtheta=0.003 * (i - 3), growth=6e-8)
           for i, a in enumerate((0, 3, 6, 7, 8, 9, 10, M.SYM_N * 5 + 1))]
    add("position a", pos[:3]); add("position b", pos[3:6]); add("position c", pos[6:])
    win = _gauss(40, 9000.0, n=BLOCK + 1080)
    add("position fifo", [_case("fifo a00 %d" % a, "fifo", win, a00=a, theta=-0.2, dtheta=-0.0131, growth=-6e-8) for a in (0, 1, 1080)])
    # exact
    rec, arb = tables()
    add("exact", [_case("exact recurrence fifo", "fifo", _gauss(50, 9000.0), tab=rec), _case("exact arbitrary raw", "raw", uni, a00=9, lead=12, tab=arb),
                  _case("exact arbitrary fifo low", "fifo", _gauss(51, RMS_LSB), tab=arb)])
    # inactive
    add("inactive", [_case("active 0", "fifo", _gauss(60, 9000.0), dtheta=0.01), _case("inactive 1", "raw", uni, a00=8, active=0), _case("active 2", "fifo", _gauss(61, RMS_LSB), theta=1.0)])
    # multi
    multi = [_case("multi raw", "raw", fs, a00=7, lead=4, theta=2.0, dtheta=0.2449, growth=6e-8), _case("multi fifo", "fifo", _gauss(70, RMS_LSB), theta=-1.0, dtheta=-0.0131),
             _case("multi exact", "fifo", _gauss(71, 9000.0), tab=rec)]
    add("multi", multi); add("multi ids", multi, ids=(2, 0, 1))
    return out


def q15(case):
    """the case's decimated Q15 stream, int16 [., 2]: the window itself, or the integer half-band of the capture (the oracle's, zero history)"""
    if case["kind"] == "fifo":
        return case["samples"]
    return _halfband(case["samples"].tobytes())


@functools.lru_cache(maxsize=8)
def _halfband(raw):
    return _ro(_oracle().halfband_fm_cu8(np.frombuffer(raw, dtype=np.uint8))[0])


def phasors(case, params=None):
    """the oscillator the model runs on: the table in exact mode, else the closed form of the case's (or the read-back) parameters"""
    if case["tab"] is not None:
        return M.table_phasors(case["tab"])
    p = params or case
    return M.phasors(p["theta"], p["dtheta"], p["growth"])


_MODEL = {}


def model(case, params=None):
    """-> (bins complex128 [32, 534], bound float64 [32]) of a case; with params (a00, theta, dtheta, growth read back from the hook) on those instead"""
    key = case["name"] if params is None else None
    if key in _MODEL:
        return _MODEL[key]
    bins, weight = M.transform(q15(case), (params or case)["a00"], phasors(case, params))
    bound = SYM_FACTOR * SYM_ERR_MEASURED * np.abs(bins).max(axis=1)
    if case["tab"] is None:
        bound = bound + P_ERR * weight
    res = (_ro(bins), _ro(bound))
    if key is not None:
        _MODEL[key] = res
    return res


def stream_args(case, kind=None):
    """the case as a stream of Engine.stage_symbols (params_mode 0); kind "fifo" on a capture case: the FIFO window that holds its half-band"""
    d = dict(a00=case["a00"], theta=case["theta"], dtheta=case["dtheta"], growth=case["growth"], active=case["active"], nco_mode=0)
    if (kind or case["kind"]) == "raw":
        d.update(raw=case["samples"], lead=case["lead"])
    else:
        d.update(q15=q15(case))
    if case["tab"] is not None:
        d.update(nco_tab=case["tab"], nco_mode=1)
    return d


# ---- params_mode 1: FINE states ----------------------------------------------------------------------------------------------------------------------
WIN_N = 71280


@functools.lru_cache(maxsize=None)
def prepare_streams():
    """three FINE streams (dicts for Engine.stage_symbols, params_mode 1) and the cases (samples only) they run on"""
    uni = _capture("uniform", 9 + WIN_N)
    sets = ((_case("prepare fifo +10", "fifo", _gauss(80, 9000.0, n=5 + WIN_N)), dict(samperr=10, cfo=0, angle=0.013, prev_angle=-0.4, theta=1.1, rd=5, wr=5 + WIN_N)),
            (_case("prepare raw -10", "raw", uni, lead=8), dict(samperr=-10, cfo=3, angle=-0.02, prev_angle=0.25, theta=-2.9, rd=9, wr=9 + WIN_N)),
            (_case("prepare fifo low -3", "fifo", _gauss(81, RMS_LSB, n=WIN_N)), dict(samperr=10, cfo=-3, angle=0.007, prev_angle=0.1, theta=0.0, rd=0, wr=WIN_N)))
    streams = []
    for c, st in sets:
        d = dict(st)
        if c["kind"] == "raw":
            d.update(raw=c["samples"], lead=c["lead"])
        else:
            d.update(q15=c["samples"])
        streams.append(d)
    return tuple(streams), tuple(c for c, _ in sets)
