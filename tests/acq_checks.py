"""Exact checks of coarse acquisition -- the stage that decides where a symbol starts -- through the nrsc5hip_stage_acquire* hooks, which run the
PRODUCTION launches on caller windows; shared by tests/test_acquire_stage_cpu.py (the CPU-emulated twin) and tests/test_gpu_acquire_stage.py (the
gfx950 code):

  stage_acquire      launch_acquire on FIFO windows: k_acq_list, k_acq_fir (tb.acq_q15), k_acq_corr, k_acq_peak (tb.shape)  = oracle.fir32_fm, cp_correlate_fm
  stage_acquire_raw  the same on attached cu8 captures, k_acq_decimate (st.rd + t, the acq_win slab) in front             = halfband_fm_cu8 sliced at rd, then those two
  stage_am_acquire   launch_am_step: the first section of k_am_block<256> / <512> (tb.am_acq_q15, tb.am_shape)            = oracle.am_fir32, cp_correlate_am

What is compared, per stream: the filtered window, the decimated window (raw seam) and the FIR history afterwards as integers; the 2160 correlation
sums and the peak as the uint32 patterns of their floats; samperr.  There is no tolerance anywhere: the build has -ffp-contract=off, no libm is
involved, the kernels state the reference's order of operations and (float) / 32767.0f is a correctly rounded division on both sides, so bit equality
is what k_acquire.hip promises.  The AM kernel keeps filtered window and sums in LDS: its peak's 64 bits are the checksum of everything before them.
A stream the acquisition must skip (FINE, or short of a window) must still show the hook's fill pattern everywhere, and its history as it went in.

The end-to-end tests cannot see a defect here.  A samperr that is off by a sample or two still locks -- the fine loop pulls it in -- and what then
differs from the reference fits the 1e-4 float tolerance and the false-lock exemptions of the capture tests.  No capture reaches the int16
accumulator's wrap (synthetic captures are 20 LSB rms), best_i < 15, the candidates whose sliding sum wraps, an exact tie, or more than 32
un-synchronised streams in a known slot of the compacted list.

If a check finds a difference: the twins are the very functions the whole-path oracle calls (oracle/nrsc5_oracle.c and nrsc5_oracle_am.c:
process_window -> orc_fir32_fm / orc_am_fir32 and the static cp_correlate behind orc_cp_correlate_*), and the golden traces under tests/golden/ pin
that path to the unmodified reference's acquire.c.  The message names the first differing stream and index with both values -- filt first (the
FIR, acquire.c:122-127 / firdecim_q15.c:95-109), then sums (acquire.c:129-134), then the peak (acquire.c:136-151): the first stage that differs is
the one to read against those lines."""
import functools

import numpy as np

from nrsc5_amd import engine as eng
from tests import acq_args as aa

EINVAL = -1
FILL16, FILL32 = np.int16(-23131), np.uint32(0xA5A5A5A5)       # the hooks' fill: 0xA5 bytes
WIN_FM = aa.GEO["fm"].win


def make_engine(lib, seam, n=1):
    """one engine per seam: "fifo", "raw" (zero-copy batch), "am" (in order: k_am_block<256>), "am-pipe" (window pipeline: k_am_block<512>)"""
    if seam == "fifo":
        return eng.Engine(max_streams=n, q15_capacity=2 * WIN_FM, lib_path=lib)
    if seam == "raw":
        return eng.Engine(max_streams=n, q15_capacity=2 * WIN_FM, p1_async=True, batch_zero_copy=True, lib_path=lib)
    E = eng.Engine(max_streams=1, q15_capacity=2 * WIN_FM, am_enable=True, p1_async=seam == "am-pipe", lib_path=lib)
    E.set_mode(0, eng.MODE_AM)
    return E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first(bad):
    return int(np.flatnonzero(np.asarray(bad).reshape(-1))[0])


# ---- the twins, once per set ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_single(mode, name):
    st = aa.single(mode, name)
    return aa.twin(mode, st.win, st.hist)


def ref_single(oracle, mode, name):
    aa.use(oracle)
    return _ref_single(mode, name)


@functools.lru_cache(maxsize=None)
def _ref_list(n):
    return tuple(aa.twin("fm", st.win, st.hist) if st.state != aa.FINE and st.fill == WIN_FM else None for st in aa.list_streams(n))


@functools.lru_cache(maxsize=None)
def _ref_raw():
    iq, rd, hist, state = aa.raw_streams()
    out = []
    for k in range(iq.shape[0]):
        win = aa._ORACLE.halfband_fm_cu8(iq[k])[0][rd[k]:rd[k] + WIN_FM]       # the whole capture from its start (zero history), sliced at rd
        out.append(dict(aa.twin("fm", win, hist[k]), acq_win=win) if state[k] != aa.FINE else None)
    return tuple(out)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------------
def compare(mode, got, exp, hists, what=""):
    """got: a hook's dict of arrays [n, ..]; exp: per stream the twin's dict, or None for a stream the acquisition must skip; hists: what went in"""
    g = aa.GEO[mode]
    for s, e in enumerate(exp):
        tag = "%s%s stream %d" % (what, mode, s)
        if e is None:
            for key in ("filt", "acq_win"):
                if key in got:
                    bad = got[key][s] != FILL16
                    assert not bad.any(), "%s is not active, yet %s[%d] was written: %d" % (tag, key, _first(bad) // 2, got[key][s].reshape(-1)[_first(bad)])
            if "sums" in got:
                bad = _bits(got["sums"][s]) != FILL32
                assert not bad.any(), "%s is not active, yet sums[%d] was written" % (tag, _first(bad) // 2)
            assert got["samperr"][s].view(np.uint32) == FILL32 and (_bits(got["peak"][s]) == FILL32).all(), "%s is not active, yet samperr / peak were written: %d, %s" % (
                tag, got["samperr"][s], got["peak"][s])
            assert np.array_equal(got["hist_out"][s], hists[s]), "%s is not active, yet its FIR history changed" % tag
            continue
        for key in ("acq_win", "filt"):                                        # integers
            if key in got:
                bad = got[key][s] != e[key]
                assert not bad.any(), "%s: %s[%d] (%s) is %d, the twin's %d (%d of %d differ)" % (
                    tag, key, _first(bad) // 2, "ri"[_first(bad) % 2], got[key][s].reshape(-1)[_first(bad)], e[key].reshape(-1)[_first(bad)], bad.sum(), bad.size)
        if "sums" in got:                                                      # the floats' bits
            bad = _bits(got["sums"][s]) != _bits(e["sums"])
            assert not bad.any(), "%s: sums[%d] (%s) is %r (0x%08x), the twin's %r (0x%08x) (%d of %d differ)" % (
                tag, _first(bad) // 2, "ri"[_first(bad) % 2], got["sums"][s].reshape(-1)[_first(bad)], _bits(got["sums"][s]).reshape(-1)[_first(bad)],
                e["sums"].reshape(-1)[_first(bad)], _bits(e["sums"]).reshape(-1)[_first(bad)], bad.sum(), bad.size)
        assert got["samperr"][s] == e["samperr"], "%s: samperr %d (best_i %d), the twin's %d (best_i %d)" % (
            tag, got["samperr"][s], aa.best_of(mode, int(got["samperr"][s])) if 0 <= got["samperr"][s] < g.sym else -1, e["samperr"], e["best_i"])
        bad = _bits(got["peak"][s]) != _bits(e["peak"])
        assert not bad.any(), "%s: peak %r (0x%08x 0x%08x), the twin's %r (0x%08x 0x%08x), best_i %d" % (
            tag, got["peak"][s], *_bits(got["peak"][s]), e["peak"], *_bits(e["peak"]), e["best_i"])
        bad = got["hist_out"][s] != e["hist_out"]
        assert not bad.any(), "%s: history[%d] afterwards is %d, the window's last 31 samples hold %d" % (
            tag, _first(bad) // 2, got["hist_out"][s].reshape(-1)[_first(bad)], e["hist_out"].reshape(-1)[_first(bad)])


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def check_single(E, oracle, mode, name):
    """one set of one stream through the seam's hook, against the twins"""
    aa.use(oracle)
    st = aa.single(mode, name)
    exp = ref_single(oracle, mode, name)
    assert np.array_equal(exp["hist_out"], st.win[-31:])                       # (the twin's history afterwards IS the window's last 31 samples)
    if mode == "am":
        got = E.stage_am_acquire(st.win, st.hist, st.state, st.fill)
    else:
        got = E.stage_acquire(st.win[None], st.hist[None], [st.state], [st.fill])
    compare(mode, got, [exp], [st.hist], what=name + ": ")
    return exp


def check_inactive(E, mode):
    """a FINE stream, and one that is a sample short of a window: nothing is written"""
    st = aa.noise(mode)
    for state, fill in ((aa.FINE, st.fill), (aa.NONE, st.fill - 1), (aa.COARSE, 0)):
        if mode == "am":
            got = E.stage_am_acquire(st.win, st.hist, state, fill)
        else:
            got = E.stage_acquire(st.win[None], st.hist[None], [state], [fill])
        compare(mode, got, [None], [st.hist], what="state %d fill %d: " % (state, fill))


def check_list(E, oracle, n=aa.LIST_N):
    """n streams in one launch: every active stream equals the twin on ITS window (a skipped, doubled or misplaced list entry shows as a stream that
    still holds the fill pattern or another stream's results), every inactive one is untouched -> (active, n)"""
    aa.use(oracle)
    streams = aa.list_streams(n)
    exp = _ref_list(n)
    got = E.stage_acquire(np.stack([st.win for st in streams]), np.stack([st.hist for st in streams]), [st.state for st in streams], [st.fill for st in streams])
    compare("fm", got, exp, [st.hist for st in streams], what="list of %d: " % n)
    return sum(e is not None for e in exp), n


def check_raw(E, oracle):
    aa.use(oracle)
    iq, rd, hist, state = aa.raw_streams()
    got = E.stage_acquire_raw(iq, rd, hist, state)
    compare("fm", got, _ref_raw(), list(hist), what="raw: ")


# ---- rejections ----------------------------------------------------------------------------------------------------------------------------
def _rc(E, fn, *args):
    return fn(E._h, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])


def check_rejections_fifo(E):
    """E: the FIFO engine (FM streams).  NRSC5HIP_EINVAL, and the next good call still works (nothing was left half done)"""
    st = aa.zero("fm")
    win, hist = np.ascontiguousarray(st.win[None]), np.ascontiguousarray(st.hist[None])
    one, full = np.array([aa.NONE], dtype=np.int32), np.array([WIN_FM], dtype=np.int32)
    o = E._acq_outputs(1)
    outs = [o[k] for k in ("filt", "sums", "samperr", "peak", "hist_out")]
    good = [1, win, hist, one, full] + outs
    fn = E.lib.nrsc5hip_stage_acquire
    assert _rc(E, fn, *good) == 0
    for k in range(1, len(good)):                                              # every pointer
        args = list(good); args[k] = None
        assert _rc(E, fn, *args) == EINVAL, k
    for n in (0, -1, E.max_streams + 1):
        args = list(good); args[0] = n
        assert _rc(E, fn, *args) == EINVAL, n
    for bad_state in (-1, 3):
        assert _rc(E, fn, 1, win, hist, np.array([bad_state], dtype=np.int32), full, *outs) == EINVAL
    for bad_fill in (-1, WIN_FM + 1):
        assert _rc(E, fn, 1, win, hist, one, np.array([bad_fill], dtype=np.int32), *outs) == EINVAL
    # the zero-copy hook needs a zero-copy engine; the AM hook an AM engine
    se, pk, ho = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.float32), np.zeros((31, 2), dtype=np.int16)
    rd = np.zeros(1, dtype=np.int64)
    iq = np.zeros(4 * WIN_FM, dtype=np.uint8)
    assert _rc(E, E.lib.nrsc5hip_stage_acquire_raw, 1, iq, iq.size, rd, hist, one, E._acq_outputs(1, raw=True)["acq_win"], *outs) == EINVAL
    assert _rc(E, E.lib.nrsc5hip_stage_am_acquire, np.zeros((aa.GEO["am"].win, 2), dtype=np.int16), hist, aa.NONE, aa.GEO["am"].win, se, pk, ho) == EINVAL
    assert _rc(E, fn, *good) == 0 and o["samperr"][0] == 2145


def check_rejections_raw(E):
    iq, rd, hist, state = aa.raw_streams()
    iq, rd, hist, state = np.ascontiguousarray(iq[:1]), rd[:1].copy(), np.ascontiguousarray(hist[:1]), state[:1].copy()
    o = E._acq_outputs(1, raw=True)
    outs = [o[k] for k in ("acq_win", "filt", "sums", "samperr", "peak", "hist_out")]
    good = [1, iq, iq.size, rd, hist, state] + outs
    fn = E.lib.nrsc5hip_stage_acquire_raw
    assert _rc(E, fn, *good) == 0
    for k in (1, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        args = list(good); args[k] = None
        assert _rc(E, fn, *args) == EINVAL, k
    for n in (0, E.max_streams + 1):
        args = list(good); args[0] = n
        assert _rc(E, fn, *args) == EINVAL, n
    last = iq.size // 4 - WIN_FM                                               # the last read position whose window the capture holds
    for bad_rd in (-1, last + 1):
        args = list(good); args[3] = np.array([bad_rd], dtype=np.int64)
        assert _rc(E, fn, *args) == EINVAL, bad_rd
    args = list(good); args[3] = np.array([last], dtype=np.int64)
    assert _rc(E, fn, *args) == 0
    for bad_len in (iq.size - 2, 0):
        args = list(good); args[2] = bad_len
        assert _rc(E, fn, *args) == EINVAL, bad_len
    args = list(good); args[5] = np.array([7], dtype=np.int32)
    assert _rc(E, fn, *args) == EINVAL
    assert _rc(E, fn, *good) == 0


def check_rejections_am(E):
    """E: an AM engine whose stream 0 is in AM mode"""
    st = aa.zero("am")
    win, hist = np.ascontiguousarray(st.win), np.ascontiguousarray(st.hist)
    se, pk, ho = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.float32), np.zeros((31, 2), dtype=np.int16)
    good = [win, hist, aa.NONE, aa.GEO["am"].win, se, pk, ho]
    fn = E.lib.nrsc5hip_stage_am_acquire
    assert _rc(E, fn, *good) == 0 and se[0] == 255
    for k in (0, 1, 4, 5, 6):
        args = list(good); args[k] = None
        assert _rc(E, fn, *args) == EINVAL, k
    for bad_state in (-1, 3):
        args = list(good); args[2] = bad_state
        assert _rc(E, fn, *args) == EINVAL
    for bad_fill in (-1, aa.GEO["am"].win + 1):
        args = list(good); args[3] = bad_fill
        assert _rc(E, fn, *args) == EINVAL
    # an AM stream is not the FM hook's, and back in FM mode the stream is not the AM hook's
    fm = aa.zero("fm")
    o = E._acq_outputs(1)
    fm_args = [1, np.ascontiguousarray(fm.win[None]), np.ascontiguousarray(fm.hist[None]), np.array([aa.NONE], dtype=np.int32), np.array([WIN_FM], dtype=np.int32)] + \
              [o[k] for k in ("filt", "sums", "samperr", "peak", "hist_out")]
    assert _rc(E, E.lib.nrsc5hip_stage_acquire, *fm_args) == EINVAL
    E.set_mode(0, eng.MODE_FM)
    try:
        assert _rc(E, fn, *good) == EINVAL
        assert _rc(E, E.lib.nrsc5hip_stage_acquire, *fm_args) == 0 and o["samperr"][0] == 2145
    finally:
        E.set_mode(0, eng.MODE_AM)
    assert _rc(E, fn, *good) == 0


# ---- what the input sets hold (no device involved) -----------------------------------------------------------------------------------------------
def check_set(oracle, mode, name):
    """the condition a set is named for, on the twin alone"""
    g = aa.GEO[mode]
    aa.use(oracle)
    st = aa.single(mode, name)
    tw = ref_single(oracle, mode, name)
    mag = tw["mag"].view(np.uint32)                                            # (non-negative floats order as their bit patterns do)
    assert st.win.shape == (g.win, 2) and st.hist.shape == (31, 2) and st.fill == g.win and st.state in (aa.NONE, aa.COARSE)
    assert tw["samperr"] == (tw["best_i"] + g.sym - 15) % g.sym
    if name == "zero":
        assert not tw["sums"].any() and not tw["filt"].any() and tw["best_i"] == 0 and tw["samperr"] == {"fm": 2145, "am": 255}[mode]
    elif name in ("fullscale", "noise"):
        x = np.concatenate([st.hist, st.win])
        assert x.min() == -32768 and x.max() == 32767
        counts = np.bincount((x.reshape(-1).astype(np.int64) + 32768) >> 12, minlength=16)      # uniform: sixteen equal slices of the range, within 6 sigma
        assert np.abs(counts - x.size / 16).max() < 6 * np.sqrt(x.size / 16)
        wrapped = (aa.fir_unwrapped(mode, st.win, st.hist) != tw["filt"]).mean()
        if name == "fullscale":
            assert wrapped >= 0.01, wrapped                                    # (measured: FM 0.35, AM 0.056)
        elif mode == "fm":
            assert 0.002 < wrapped < 0.01, wrapped
    elif name.startswith("rails-"):
        v = -32768 if name == "rails-lo" else 32767
        assert (st.win == v).all() and (st.hist == v).all()
        q = aa.acq_taps(mode)
        assert 2 ** 28 < max(abs(2 * v * t) for t in q) < 2 ** 31                # (xa + xb) * q: the largest int products the filter can see
        assert (mag == mag[0]).all() and tw["best_i"] == 0                     # a constant window: every candidate ties, the first wins
    elif name.startswith("peak@"):
        p, amp = name[5:].split("-")
        assert tw["best_i"] == int(p) and (mag[:int(p)] < mag[int(p)]).all() and (mag[int(p) + 1:] <= mag[int(p)]).all()
        assert np.abs(st.win).max() == 1 if amp == "lsb" else 1500 < st.win.astype(np.float64).std() < 3500
    else:
        period, first = aa.TIES[mode][name[5:]]
        at = np.arange(first, g.sym, period)
        assert tw["best_i"] == first and at.size == g.sym // period
        assert (mag[at] == mag[first]).all(), "the maxima differ in their bits"
        rest = np.delete(mag, at)
        assert (rest < mag[first]).all()
        assert np.array_equal(_bits(tw["sums"])[:period], _bits(tw["sums"])[period:2 * period])
        lanes = at % 256
        if (mode, name[5:]) == ("fm", "wave"):
            assert first % 256 < 228 and lanes[0] // 64 == lanes[1] // 64 == lanes[2] // 64
        if (mode, name[5:]) == ("fm", "lane"):
            assert first % 256 >= 228 and lanes[1] < lanes[0]
        if (mode, name[5:]) == ("am", "pass2"):
            assert at[-1] >= 256 and at[-1] - 256 < 14                         # the second pass of lanes 0 .. 13 (256-lane form) holds a maximum
        if (mode, name[5:]) == ("am", "wave"):
            assert lanes[0] // 64 == lanes[1] // 64


def check_set_list(n=aa.LIST_N):
    streams = aa.list_streams(n)
    state, fill = np.array([st.state for st in streams]), np.array([st.fill for st in streams])
    active = aa.list_active(state, fill)
    assert (state[::5] == aa.FINE).all() and (fill[::7] == WIN_FM - 1).all() and set(state[active]) == {aa.NONE, aa.COARSE}
    assert len({st.win.tobytes() for st in streams}) == n and len({st.hist.tobytes() for st in streams}) == n      # distinct windows and histories
    return int(active.sum())


def check_set_raw(oracle):
    aa.use(oracle)
    iq, rd, hist, state = aa.raw_streams()
    assert tuple(rd[:3]) == (0, 5, 4321) and (state[:3] != aa.FINE).all() and state[3] == aa.FINE
    assert all(np.unique(c).size == 256 for c in iq) and 4 * (rd.max() + WIN_FM) == iq.shape[1]
    exp = _ref_raw()
    assert exp[3] is None and len({e["acq_win"].tobytes() for e in exp[:3]}) == 3
