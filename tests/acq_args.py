"""Inputs for the exact checks of coarse acquisition (tests/acq_checks.py), written once: numpy only, fixed seeds, cached, read-only.  A set is
a list of streams, each (window int16 [WIN, 2], FIR history int16 [31, 2], sync state, fill); WIN is 71280 (FM) or 8910 (AM).

  zero         all-zero window and history: every sum is zero, the first candidate wins
  fullscale    uniform over all 65536 int16 values, both rails present, shaped so that the FIR's int16 accumulator wraps in far more than 1 % of outputs
  noise        the same values as independent samples (white): what a full-scale random capture gives
  rails        both components constant -32768 / constant 32767: (xa + xb) * q at +-2^31
  peak@p       33 random symbols with their cyclic prefix, rolled until the TWIN's arg-max is candidate p, at the synthesiser's level (20 * 128 LSB
               rms) and at +-1 LSB; the p are both sides of the samperr wrap (best_i < 15), of the 256-lane stride, of the candidate from which
               the sliding sum's index wraps (SYM - CP), and the last candidate
  ties         a window of period SYM / 4 (FM: 540) or SYM / 3 (AM: 90) whose history is its periodic continuation: the sums repeat bit for bit, so
               4 (3) candidates hold the maximum.  Rotated until the first of them, m, is where a wrong tie-break shows:
                 FM "wave"  m = 70: candidates 70, 610, 1150 sit on lanes 70, 98, 126 of ONE wave (the shuffle reduction decides)
                 FM "lane"  m = 240 (m % 256 >= 228): 780 sits on lane 12, a LOWER lane than 240's (the four-wave reduction decides)
                 AM "low"   m = 40: candidates 40, 130, 220
                 AM "pass2" m = 80: candidate 260 is the SECOND pass of lane 4 in the 256-lane form
                 AM "wave"  period 30, m = 5: nine maxima, 5, 35 on lanes of one wave (with period 90 no two maxima ever share a wave)
  list         (FM FIFO seam) LIST_N streams: rolls of the peak@p windows with histories of their own; every 5th is FINE, every 7th one sample
               short of a window, the rest alternate NONE / COARSE -- at least 65 active ones, so that rows of the 32-row list walk serve three
  raw          (FM zero-copy seam) captures of uniform bytes read at rd = 0, 5, 4321, and a FINE stream

The twin (oracle/port.py: fir32_fm / cp_correlate_fm, am_fir32 / cp_correlate_am) is needed to BUILD peak@p and ties: the roll is chosen by
what the twin reports, and tests/test_acquire_stage_cpu.py asserts, under "the sets", that every set holds what its name says."""
import collections
import functools

import numpy as np

Geo = collections.namedtuple("Geo", "sym fft cp win")
GEO = {"fm": Geo(2160, 2048, 112, 71280), "am": Geo(270, 256, 14, 8910)}
NONE, COARSE, FINE = 0, 1, 2
FILTER_DELAY = 15
PEAKS = {"fm": (0, 14, 15, 255, 256, 2048, 2049, 2159), "am": (0, 13, 14, 15, 255, 256, 257, 269)}
AMPS = ("synth", "lsb")                   # 20 LSB of the 8-bit capture = 20 * 128 Q15 units rms; +-1 Q15 unit
TIES = {"fm": {"wave": (540, 70), "lane": (540, 240)}, "am": {"low": (90, 40), "pass2": (90, 80), "wave": (30, 5)}}      # name: (period, first maximum)
LIST_ACTIVE_MIN = 65
RAW_RD = (0, 5, 4321)
Stream = collections.namedtuple("Stream", "win hist state fill")

_ORACLE = None


def use(oracle):
    global _ORACLE
    _ORACLE = oracle


def _ro(a):
    a.setflags(write=False)
    return a


def best_of(mode, samperr):
    """the arg-max candidate behind a samperr (acquire.c:149: samperr = (i + SYM - FILTER_DELAY) % SYM)"""
    return (samperr + FILTER_DELAY) % GEO[mode].sym


def twin(mode, win, hist):
    """the two acquisition twins on one stream -> dict(filt, hist_out, samperr, best_i, peak float32 [2], sums float32 [SYM, 2], mag float32 [SYM])"""
    fir, cp = (_ORACLE.fir32_fm, _ORACLE.cp_correlate_fm) if mode == "fm" else (_ORACLE.am_fir32, _ORACLE.cp_correlate_am)
    filt, hist_out = fir(win, hist)
    samperr, peak, sums, mag = cp(filt, sums=True)
    return dict(filt=filt, hist_out=hist_out, samperr=samperr, best_i=best_of(mode, samperr), peak=peak, sums=sums, mag=mag)


def _levels(rng, amp, shape):
    if amp == "lsb":
        return (2 * rng.integers(0, 2, size=shape) - 1).astype(np.int16)
    return np.clip(np.rint(rng.normal(0.0, 20.0 * 128.0, size=shape)), -32768, 32767).astype(np.int16)


# ---- the plain sets ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zero(mode):
    return Stream(_ro(np.zeros((GEO[mode].win, 2), dtype=np.int16)), _ro(np.zeros((31, 2), dtype=np.int16)), NONE, GEO[mode].win)


@functools.lru_cache(maxsize=None)
def noise(mode):
    """independent samples, uniform over all 65536 int16 values.  (The FM filter's int16 accumulator wraps in 0.6 % of its outputs on this, the AM
    filter's, whose taps sum to 1.28, in none: the rms gain of either filter is below one.  fullscale is the set made to wrap.)"""
    rng = np.random.default_rng(9101 + (mode == "am"))
    win = rng.integers(-32768, 32768, size=(GEO[mode].win, 2)).astype(np.int16)
    hist = rng.integers(-32768, 32768, size=(31, 2)).astype(np.int16)
    win[100], win[101], hist[3], hist[30] = (-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767)
    return Stream(_ro(win), _ro(hist), COARSE, GEO[mode].win)


@functools.lru_cache(maxsize=None)
def fullscale(mode):
    """uniform over all 65536 int16 values, but not white: independent samples leave the filter's output inside int16 nearly everywhere (see noise),
    so the signs follow a square wave at the frequency where the filter's response peaks (read off the twin's taps) and the magnitudes a slow
    sawtooth over 0 .. 32767 -- every value equally often, every stretch of high magnitude driving the accumulator past +-2^15"""
    g = GEO[mode]
    q = acq_taps(mode)
    h = np.array([0] + [q[k] if k <= 16 else q[32 - k] for k in range(1, 32)], dtype=np.float64)
    f = np.argmax(np.abs(np.fft.rfft(h, 8192))) / 8192.0
    t = np.arange(g.win + 31)
    x = np.zeros((g.win + 31, 2), dtype=np.int16)
    for c, phase in enumerate((0.0, 0.25)):
        m = ((5 if mode == "fm" else 37) * t + 12345 * c) % 32768              # about eleven (FM) / ten (AM) sweeps of the magnitude
        x[:, c] = np.where(np.cos(2 * np.pi * (f * t + phase)) >= 0, m, -1 - m)
    x[131], x[132], x[3], x[30] = (-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767)
    return Stream(_ro(x[31:].copy()), _ro(x[:31].copy()), COARSE, g.win)


@functools.lru_cache(maxsize=None)
def rails(mode, value):
    assert value in (-32768, 32767)
    return Stream(_ro(np.full((GEO[mode].win, 2), value, dtype=np.int16)), _ro(np.full((31, 2), value, dtype=np.int16)), NONE, GEO[mode].win)


@functools.lru_cache(maxsize=None)
def acq_taps(mode):
    """int [17]: the Q15 taps, tap i applied to a[i] + a[32 - i] (16: the centre), read off the twin's answer to one sample of -32768:
    (-32768 * q) >> 15 = -q exactly, and every output holds one product only"""
    x = np.zeros((32, 2), dtype=np.int16)
    x[0, 0] = -32768
    y = (_ORACLE.fir32_fm if mode == "fm" else _ORACLE.am_fir32)(x)[0][:, 0].astype(np.int64)      # the sample is a[31 - t] of output t
    assert y[31] == 0                                                          # a[0]: the 32nd tap is zero
    return tuple([0] + [int(-y[31 - i]) for i in range(1, 17)])


def fir_unwrapped(mode, win, hist):
    """the same FIR with an int32 accumulator that never wraps (numpy int64): what the int16 one would give if it were wide enough, truncated to int16
    only at the end -- the fullscale set must differ from it"""
    taps = acq_taps(mode)
    w = np.concatenate([hist, win]).astype(np.int64)                           # a[k] of output t = w[t + k]
    n = win.shape[0]
    acc = np.zeros((n, 2), dtype=np.int64)
    for i in range(1, 16):
        acc += ((w[i:i + n] + w[32 - i:32 - i + n]) * int(taps[i])) >> 15
    acc += (w[16:16 + n] * int(taps[16])) >> 15
    return acc


# ---- windows with a cyclic prefix -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cp_window(mode, amp, variant=0):
    g = GEO[mode]
    rng = np.random.default_rng(9200 + 10 * (mode == "am") + AMPS.index(amp) + 100 * variant)
    body = _levels(rng, amp, (33, g.fft, 2))
    return _ro(np.concatenate([body[:, g.fft - g.cp:], body], axis=1).reshape(g.win, 2)), _ro(_levels(rng, amp, (31, 2)))


@functools.lru_cache(maxsize=None)
def peak_at(mode, amp, p):
    """rolled until the twin's arg-max is p (the roll moves the symbol boundary; the few samples the history and the seam change can move the
    arg-max by a candidate or two, hence the loop)"""
    g = GEO[mode]
    for variant in range(6):                                                   # (at +-1 LSB the maximum is flat: a given window may step over a candidate at every roll; the next seed then)
        base, hist = _cp_window(mode, amp, variant)
        roll, tried = 0, {}
        for step in range(16):
            win = np.roll(base, roll, axis=0)
            got = tried[roll] = twin(mode, win, hist)["best_i"]
            if got == p:
                return Stream(_ro(win), hist, COARSE if p & 1 else NONE, g.win)
            roll = (roll + p - got) % g.sym
            if roll in tried:                                                  # a cycle (two rolls whose arg-max steps over p): the untried rolls next to it
                roll = next(r % g.sym for d in range(1, 24) for r in (roll + d, roll - d) if r % g.sym not in tried)
    raise AssertionError("no roll of the %s %s windows puts the twin's arg-max at %d (last: %d)" % (mode, amp, p, got))


# ---- exact ties ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties(mode, name):
    g = GEO[mode]
    period, first = TIES[mode][name]
    assert g.sym % period == 0 and g.win % period == 0 and first < period
    base = _levels(np.random.default_rng(9300 + 10 * (mode == "am") + sorted(TIES[mode]).index(name)), "synth", (period, 2))

    def stream(b):
        return np.tile(b, (g.win // period, 1)), b[np.arange(-31, 0) % period]

    m0 = twin(mode, *stream(base))["best_i"]
    win, hist = stream(np.roll(base, first - m0, axis=0))                      # a rotation of a periodic signal: every candidate moves with it, exactly
    return Stream(_ro(win), _ro(hist), NONE, g.win)


# ---- the compacted list (FM FIFO seam) -----------------------------------------------------------------------------------------------------------
def list_pattern(n):
    state, fill = np.zeros(n, dtype=np.int32), np.full(n, GEO["fm"].win, dtype=np.int32)
    for k in range(n):
        state[k] = FINE if k % 5 == 0 else (NONE, COARSE)[k & 1]
        if k % 7 == 0:
            fill[k] -= 1
    return state, fill


def list_active(state, fill):
    return (state != FINE) & (fill == GEO["fm"].win)


def list_n(active_min=LIST_ACTIVE_MIN):
    n = 1
    while list_active(*list_pattern(n)).sum() < active_min:
        n += 1
    return n


LIST_N = list_n()                                                              # 95


@functools.lru_cache(maxsize=None)
def list_streams(n=LIST_N):
    state, fill = list_pattern(n)
    out = []
    for k in range(n):
        src = peak_at("fm", "synth", PEAKS["fm"][k % len(PEAKS["fm"])])
        hist = _levels(np.random.default_rng(9400 + k), "synth", (31, 2))
        out.append(Stream(_ro(np.roll(src.win, 37 * k + 1, axis=0)), _ro(hist), int(state[k]), int(fill[k])))
    return tuple(out)


# ---- captures (FM zero-copy seam) ---------------------------------------------------------------------------------------------------------
RAW_BYTES = 4 * (max(RAW_RD) + GEO["fm"].win)                                  # the window at the largest rd ends with the capture


@functools.lru_cache(maxsize=None)
def raw_streams():
    """-> (iq uint8 [4, RAW_BYTES], rd int64 [4], hist int16 [4, 31, 2], state int32 [4]): three active captures and a FINE one"""
    rng = np.random.default_rng(9500)
    iq = rng.integers(0, 256, size=(len(RAW_RD) + 1, RAW_BYTES), dtype=np.uint8)
    hist = _levels(rng, "synth", (len(RAW_RD) + 1, 31, 2))
    return _ro(iq), _ro(np.array(RAW_RD + (0,), dtype=np.int64)), _ro(hist), _ro(np.array([NONE, COARSE, NONE, FINE], dtype=np.int32))


def single_names(mode):
    return ["zero", "fullscale", "noise", "rails-lo", "rails-hi"] + ["peak@%d-%s" % (p, amp) for amp in AMPS for p in PEAKS[mode]] + ["ties-" + n for n in TIES[mode]]


def single(mode, name):
    if name == "zero":
        return zero(mode)
    if name == "fullscale":
        return fullscale(mode)
    if name == "noise":
        return noise(mode)
    if name.startswith("rails-"):
        return rails(mode, -32768 if name == "rails-lo" else 32767)
    if name.startswith("peak@"):
        p, amp = name[5:].split("-")
        return peak_at(mode, amp, int(p))
    return ties(mode, name[5:])
