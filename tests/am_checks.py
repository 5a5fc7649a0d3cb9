"""Checks of the AM block step -- k_am_block, the largest kernel body of the tree -- through nrsc5hip_stage_am_block, which launches the PRODUCTION kernel alone on a
caller's window and state words; shared by tests/test_am_block_stage_cpu.py (the CPU-emulated twin) and tests/test_gpu_am_block_stage.py (the gfx950 code).  The
reference is tests/am_model.py, a float64 restatement of one block that is itself pinned to the oracle's log; the inputs and every tolerance are tests/am_args.py's.

What is compared, per call:
  exact   every integer of the record and of the state; the block's 4 x 800 hard symbols at bc * 800 on every cell whose model distance to a slicer boundary exceeds
          the margin (a cell inside it: within one grid step); the 64 PIDS cells through pids_coded; next_samperr where `se` is further than its margin from a half
          integer (else within one); in order: rec.pids and the CRC flag against the oracle's K=9 decoder on the model's trellis input
  fill    the other seven blocks' cells, and for a block that does not end FINE all symbols, the staged PIDS bytes and the taps, still hold the hook's 0xA5 bytes
  floats  prev_angle, phase_re / phase_im, freq_offset, theta within tests/common.py's bounds
  tile    the dumped spectra on bins -81 .. +81 within eps = SPEC_BOUND * largest bin, the taps within |tap| eps / t (am_args.margins)
A failure names the first differing field or cell with both values and the model's distance: the first stage that differs is the one to read against am_model.block,
whose steps are numbered as the kernel's sections are ordered."""
import numpy as np

from nrsc5_amd import engine as eng
from tests import acq_checks, am_args as aa, am_model as M, common

EINVAL = -1
FILL8 = 0xA5
PIPE_ONLY = eng.REC_P1 | eng.REC_P3 | eng.REC_PIDS_CRC
GEN_E2 = (0o561, 0o753, 0o711)
REC_INTS = ("state_before", "state_after", "samperr", "cfo", "keep", "bc", "psmi", "cfo_wait", "bc_decoded", "sis")
STATE_INTS = ("sync_state", "cfo", "psmi", "bc", "cfo_wait", "coarse_samperr", "keep_extra", "offset_history", "rdbi", "pli", "hppi", "aabi", "am_diversity_wait",
              "am_errors", "fine_epoch", "active", "nblocks", "rd")
_LEVEL8 = np.argsort(np.array([0, 4, 6, 2, 3, 7, 5, 1]))       # slicer code -> index of its interval
_LEVEL4 = np.argsort(np.array([0, 2, 3, 1]))
make_engine = acq_checks.make_engine


def run(E, c, dump=True):
    """the hook's answer for a case, once per engine"""
    cache = E.__dict__.setdefault("_am_block_cache", {})
    key = (c.name, c.fill, dump, id(c))
    if key not in cache:
        cache[key] = E.stage_am_block(c.win, c.hist, c.state, c.fill, dump)
    return cache[key]


def levels(code, part, ma3):
    """[.., 2]: the interval indices (re, im) of hard-symbol codes"""
    code = np.asarray(code, dtype=np.int64)
    if part < 2 or ma3:
        return np.stack([_LEVEL8[code & 7], _LEVEL8[(code >> 3) & 7]], axis=-1)
    if part == 2:
        return np.stack([_LEVEL4[code & 3], _LEVEL4[(code >> 2) & 3]], axis=-1)
    return np.stack([code & 1, (code >> 1) & 1], axis=-1)


def _close(key, exp, got):
    return common.float_close(key, float(exp), float(got))


def compare(c, got, exp, pipeline, oracle=None, tag=""):
    """got: Engine.stage_am_block's dict; exp: am_model.block's -> the share of cells that were excluded (inside their margin)"""
    tag = "%s%s (%s)" % (tag, c.name, "k_am_block<512>, pipeline" if pipeline else "k_am_block<256>, in order")
    gs, es = got["state"], exp["state"]
    assert gs["active"] == exp["active"], "%s: st.active %d, the model's %d" % (tag, gs["active"], exp["active"])
    if not exp["active"]:
        for k in M.STATE_DEFAULTS:
            if k != "active":
                want = dict(M.STATE_DEFAULTS, **c.state)[k]
                assert gs[k] == (np.float32(want) if isinstance(want, float) and k != "theta" else want), "%s: not active, yet st.%s went from %r to %r" % (tag, k, want, gs[k])
        assert (np.frombuffer(got["rec"].tobytes(), dtype=np.uint8) == FILL8).all(), "%s: not active, yet the record was written" % tag
        for k in ("am_sym", "pids_stage", "spectra", "mult"):
            assert (np.frombuffer(got[k].tobytes(), dtype=np.uint8) == FILL8).all(), "%s: not active, yet %s was written" % (tag, k)
        return 0.0
    mg = aa.margins(exp)
    r, er = got["rec"], exp["rec"]
    # tile first: the earliest stage
    idx = np.arange(-81, 82) % M.FFT
    err = np.abs(got["spectra"].astype(np.complex128) - exp["spectra"])[:, idx]
    if err.max() > mg["eps"]:
        n, k = np.unravel_index(np.argmax(err > mg["eps"]), err.shape)
        raise AssertionError("%s: spectrum of symbol %d, bin %+d is %r, the model's %r: off by %.3g, bound %.3g (%.3g of the largest bin)" % (
            tag, n, k - 81, got["spectra"][n, idx[k]], exp["spectra"][n, idx[k]], err[n, k], mg["eps"], aa.SPEC_BOUND))
    # the integers of the record and the state
    flags = int(r["flags"]) & ~PIPE_ONLY
    assert flags == er["flags"], "%s: rec.flags 0x%x (less the pipeline's), the model's 0x%x" % (tag, flags, er["flags"])
    # the pipeline form announces what the deferred decodes deliver in this block (decode.c:507-554): a P1 frame once the diversity delay has run out, the P3 frame in block 7
    announce = pipeline and "sym" in exp and es["am_diversity_wait"] == 0
    want = (eng.REC_P1 | (eng.REC_P3 if er["bc_decoded"] == 7 and not es["rdbi"] else 0)) if announce else 0
    assert int(r["flags"]) & (eng.REC_P1 | eng.REC_P3) == want and int(r["p1_slot"]) == (0 if announce else -1), "%s: rec.flags 0x%x, p1_slot %d: the frame flags should be 0x%x" % (
        tag, r["flags"], r["p1_slot"], want)
    for k in REC_INTS:
        assert int(r[k]) == er[k], "%s: rec.%s is %d, the model's %d (refmask 0x%08x, nearest reference bit %.3g from zero)" % (tag, k, r[k], er[k], exp["refmask"], exp["ref_dist"])
    for k in STATE_INTS:
        assert gs[k] == es[k], "%s: st.%s is %d, the model's %d" % (tag, k, gs[k], es[k])
    if c.state.get("sync_state", M.NONE) != M.FINE:
        peak = complex(es["coarse_re"], es["coarse_im"])
        assert abs(complex(gs["coarse_re"], gs["coarse_im"]) - peak) <= 1e-4 * abs(peak), "%s: the correlation peak is %r, the model's %r" % (tag, (gs["coarse_re"], gs["coarse_im"]), peak)
    else:
        assert (gs["coarse_re"], gs["coarse_im"]) == (np.float32(es["coarse_re"]), np.float32(es["coarse_im"])), "%s: a FINE block wrote the coarse peak" % tag
    assert gs["angle"] == np.float32(es["angle"]), "%s: st.angle is %r, the model's %r" % (tag, gs["angle"], es["angle"])
    for k in ("mer_lb", "mer_ub", "ber", "next_angle"):
        assert float(r[k]) == (es["angle"] if k == "next_angle" else 0.0), "%s: rec.%s is %r" % (tag, k, r[k])
    # floats
    for k in ("prev_angle", "phase_re", "phase_im", "freq_offset"):
        assert _close(k, er[k], r[k]), "%s: rec.%s is %r, the model's %r" % (tag, k, r[k], er[k])
    assert _close("prev_angle", es["prev_angle"], gs["prev_angle"]), "%s: st.prev_angle is %r, the model's %r" % (tag, gs["prev_angle"], es["prev_angle"])
    dth = abs(M.wrap(gs["theta"] - es["theta"]))
    assert dth <= common.ABS_ONLY["phase_re"], "%s: st.theta is %r, the model's %r" % (tag, gs["theta"], es["theta"])
    share = 0.0
    sym = got["am_sym"].reshape(4, 8, 800)
    if "sym" not in exp:
        for k in ("am_sym", "pids_stage", "mult"):
            assert (np.frombuffer(got[k].tobytes(), dtype=np.uint8) == FILL8).all(), "%s: the block does not end FINE, yet %s was written" % (tag, k)
        assert gs["samperr"] == es["samperr"] and int(r["next_samperr"]) == er["next_samperr"], "%s: st.samperr is %d, the model's %d" % (tag, gs["samperr"], es["samperr"])
        assert not r["pids"].any() and int(r["p1_slot"]) == -1, "%s: the block does not end FINE, yet rec.pids / p1_slot were written" % tag
        return share
    ma3 = er["psmi"] == M.MA3
    bc = er["bc_decoded"]
    # the taps
    terr = np.abs(got["mult"].astype(np.complex128) - exp["mult"])
    tbound = np.abs(exp["mult"]) * mg["eps"] / exp["train"] + 4e-7 * np.abs(exp["mult"])             # (+ the float32 rounding of the dumped tap itself)
    if (terr > tbound).any():
        p, col = np.unravel_index(np.argmax(terr > tbound), terr.shape)
        raise AssertionError("%s: equaliser tap of partition %d, column %d is %r, the model's %r: off by %.3g, bound %.3g" % (tag, p, col, got["mult"][p, col], exp["mult"][p, col], terr[p, col], tbound[p, col]))
    # the timing estimate
    if exp["wrap_dist"] > mg["wrap"] and exp["se_dist"] > mg["se"]:
        assert gs["samperr"] == es["samperr"], "%s: next samperr is %d, the model's %d (se %.6f, %.3g from a half integer, margin %.3g)" % (tag, gs["samperr"], es["samperr"], exp["se"], exp["se_dist"], mg["se"])
    else:
        assert exp["wrap_dist"] > mg["wrap"] and abs(gs["samperr"] - es["samperr"]) <= 1, "%s: next samperr is %d, the model's %d (se %.6f)" % (tag, gs["samperr"], es["samperr"], exp["se"])
    assert int(r["next_samperr"]) == gs["samperr"], "%s: rec.next_samperr %d, st.samperr %d" % (tag, r["next_samperr"], gs["samperr"])
    # the cells
    other = np.delete(sym, bc, axis=1)
    assert (other == FILL8).all(), "%s: a cell of another block than %d was written: partition %d, block %d" % (tag, bc, *[int(v[0]) for v in np.nonzero(other != FILL8)[:2]])
    mine = sym[:, bc]
    out_cell, out_pids = aa.excluded(exp, mg)
    bad = (mine != exp["sym"]) & ~out_cell
    if bad.any():
        p, k = np.unravel_index(np.argmax(bad), bad.shape)
        raise AssertionError("%s: partition %d, symbol %d, column %d is sliced to %d, the model's %d; the model's distance to a boundary %.4g grid units, margin %.4g (%d cells differ)" % (
            tag, p, k // 25, k % 25, mine[p, k], exp["sym"][p, k], exp["dist"][p, k], mg["cell"][p, 0], bad.sum()))
    for p in range(4):
        step = np.abs(levels(mine[p], p, ma3) - levels(exp["sym"][p], p, ma3)).max(axis=-1)
        assert (step <= 1).all(), "%s: partition %d, cell %d is more than one grid step from the model's: %d vs %d" % (tag, p, int(np.argmax(step > 1)), mine[p][np.argmax(step > 1)], exp["sym"][p][np.argmax(step > 1)])
    share = float(out_cell.mean())
    # the PIDS carriers, through the gathered trellis input
    if pipeline:
        coded = got["pids_stage"]
        assert not r["pids"].any() and not (int(r["flags"]) & eng.REC_PIDS_CRC), "%s: the pipeline form decoded the PIDS frame in the block step" % tag
    else:
        assert (got["pids_stage"].view(np.uint8) == FILL8).all(), "%s: the in-order form staged a PIDS frame" % tag
        coded = None
    if not out_pids.any():
        if coded is not None:
            bad = coded != exp["pids_coded"]
            assert not bad.any(), "%s: pids_coded[%d] is %d, the model's %d (%d differ; nearest PIDS cell %.4g from a boundary)" % (
                tag, int(np.argmax(bad)), coded[np.argmax(bad)], exp["pids_coded"][np.argmax(bad)], bad.sum(), exp["pids_dist"].min())
        elif oracle is not None:
            bits = oracle.descramble(oracle.viterbi(exp["pids_coded"], 9, GEN_E2))
            words = np.packbits(np.concatenate([bits, np.zeros(16, dtype=np.uint8)]), bitorder="little").view("<u4")
            assert np.array_equal(r["pids"], words), "%s: rec.pids is %s, the oracle's decode of the model's trellis input %s" % (tag, r["pids"], words)
            crc = bool(int(r["flags"]) & eng.REC_PIDS_CRC)
            assert crc == oracle.pids_crc_ok(bits), "%s: REC_PIDS_CRC is %d, pids_crc_ok says %d" % (tag, crc, not crc)
    return share


def check_case(E, oracle, which, name):
    c = aa.case(which, name)
    exp = aa.expected(which, name)
    pipeline = bool(E.cfg.p1_async)
    share = compare(c, run(E, c), exp, pipeline, oracle, tag=which + ": ")
    print("%s/%s: %.3f %% of the cells excluded" % (which, name, 100 * share))
    assert share == 0.0 if which != "edge" else share <= 0.01, (which, name, share)
    return share


def _same(a, b, what, tag):
    assert a.tobytes() == b.tobytes(), "%s: %s differs, first at byte %d" % (tag, what, int(np.argmax(np.frombuffer(a.tobytes(), dtype=np.uint8) != np.frombuffer(b.tobytes(), dtype=np.uint8))))


def check_shapes(E256, E512, which):
    """<256> and <512> leave byte-identical symbols, spectra, taps, records (less the pipeline-only flags, p1_slot and the decoded PIDS words) and state"""
    for c in aa.SETS[which]():
        a, b = run(E256, c), run(E512, c)
        tag = "%s/%s, <256> vs <512>" % (which, c.name)
        for k in ("am_sym", "spectra", "mult"):
            _same(a[k], b[k], k, tag)
        ra, rb = a["rec"].copy(), b["rec"].copy()
        for r in (ra, rb):
            if r["flags"] != 0xA5A5A5A5:
                r["flags"] &= ~np.uint32(PIPE_ONLY); r["p1_slot"] = -1; r["pids"] = 0
        _same(ra, rb, "the record", tag)
        for k in a["state"]:
            assert np.array_equal(np.array(a["state"][k]).tobytes(), np.array(b["state"][k]).tobytes()), "%s: st.%s is %r and %r" % (tag, k, a["state"][k], b["state"][k])


def check_dump(E, which):
    """DUMP = true and false leave byte-identical outputs"""
    for c in aa.SETS[which]():
        a, b = run(E, c, True), run(E, c, False)
        tag = "%s/%s, DUMP true vs false" % (which, c.name)
        for k in ("am_sym", "pids_stage"):
            _same(a[k], b[k], k, tag)
        _same(a["rec"], b["rec"], "the record", tag)
        assert a["state"] == b["state"] or all(np.array(a["state"][k]).tobytes() == np.array(b["state"][k]).tobytes() for k in a["state"]), "%s: the state differs" % tag
        assert "spectra" not in b


def check_rejections(E):
    """E: an AM engine whose stream 0 is in AM mode.  NRSC5HIP_EINVAL, nothing launched, and the next good call still works"""
    c = aa.cells()[0]
    fn = E.lib.nrsc5hip_stage_am_block
    win, hist = np.ascontiguousarray(c.win), np.ascontiguousarray(c.hist)
    rec, sym, stage = np.zeros(1, dtype=eng.RECORD_DTYPE), np.zeros((4, 6400), dtype=np.uint8), np.zeros(240, dtype=np.int8)
    spectra, mult = np.zeros((32, 256), dtype=np.complex64), np.zeros((4, 25), dtype=np.complex64)
    import ctypes

    def call(state=None, fill=M.WIN, dump=1, drop=()):
        sin, sout = eng.AmBlockState(**dict(dict(psmi=1, am_diversity_wait=4), **(c.state if state is None else state))), eng.AmBlockState()
        args = [win.ctypes.data, hist.ctypes.data, ctypes.byref(sin), fill, dump, rec.ctypes.data, ctypes.byref(sout), sym.ctypes.data, stage.ctypes.data, spectra.ctypes.data,
                mult.ctypes.data]
        for k in drop:
            args[k] = None
        return fn(E._h, *args)
    assert call() == 0 and rec[0]["state_after"] == M.FINE
    for k in (0, 1, 2, 5, 6, 7, 8, 9, 10):
        assert call(drop=(k,)) == EINVAL, k
    assert call(dump=0, drop=(9, 10)) == 0                                     # the dump buffers may be null without a dump
    for bad in (dict(sync_state=-1), dict(sync_state=3), dict(bc=-1), dict(bc=8), dict(samperr=-136), dict(samperr=136), dict(coarse_samperr=-1), dict(coarse_samperr=270)):
        assert call(state=dict(c.state, **bad)) == EINVAL, bad
    for bad_fill in (-1, M.WIN + 1):
        assert call(fill=bad_fill) == EINVAL, bad_fill
    out = np.zeros((4, 6400), dtype=np.uint8)
    assert E.lib.nrsc5hip_debug_fetch_am_sym(E._h, 0, None) == EINVAL and E.lib.nrsc5hip_debug_fetch_am_sym(E._h, 1, out.ctypes.data) == EINVAL
    E.set_mode(0, eng.MODE_FM)
    try:
        assert call() == EINVAL                                               # an FM-mode stream
    finally:
        E.set_mode(0, eng.MODE_AM)
    assert call() == 0 and rec[0]["state_after"] == M.FINE
    assert E.lib.nrsc5hip_debug_fetch_am_sym(E._h, 0, out.ctypes.data) == 0 and not out.any()      # the hook left the matrices as the engine's creation does


def check_rejects_engine_without_am(lib):
    E = eng.Engine(max_streams=1, q15_capacity=2 * acq_checks.WIN_FM, lib_path=lib)
    try:
        c = aa.cells()[0]
        try:
            E.stage_am_block(c.win, c.hist, c.state)
        except eng.Nrsc5HipError:
            pass
        else:
            raise AssertionError("an engine without am_enable ran the AM block step")
        assert E.lib.nrsc5hip_debug_fetch_am_sym(E._h, 0, np.zeros((4, 6400), dtype=np.uint8).ctypes.data) == EINVAL
    finally:
        E.close()


# ---- what the sets hold, on the model alone ---------------------------------------------------------------------------------------------------------
def check_set(which, name):
    c = aa.case(which, name)
    exp = aa.expected(which, name)
    assert c.win.shape == (M.WIN, 2) and c.win.dtype == np.int16 and c.hist.shape == (31, 2)
    if which == "inactive":
        assert c.fill < M.WIN and not exp["active"] and "rec" not in exp
        return
    mg = aa.margins(exp)
    rms = np.sqrt((c.win.astype(np.float64) ** 2).sum(axis=1).mean())
    if name == "fullscale":
        assert np.abs(c.win).max() >= 31999
    else:
        assert 19.0 < rms < 21.0, rms
    assert exp["ref_dist"] > 2 * mg["eps"], "a reference bit within the spectrum bound of zero"
    if "acq_ratio" in exp:
        assert exp["acq_ratio"] >= 1 + 1e-4, exp["acq_ratio"]                  # the correlation's arg-max: float32 sums of 448 terms are within 1e-5 of the float64 ones
    st, er, es = dict(M.STATE_DEFAULTS, **c.state), exp["rec"], exp["state"]
    if "sym" in exp:
        out_cell, out_pids = aa.excluded(exp, mg)
        share = out_cell.mean()
        assert exp["wrap_dist"] > 2 * mg["wrap"], "a tap-angle difference within its bound of a wrap threshold"
        assert not out_pids.any(), "a PIDS cell within its margin"
        assert mg["cell"].max() < 0.05, mg["cell"]
        if which == "edge":
            assert aa.EDGE_SHARE[0] <= share <= aa.EDGE_SHARE[1], share
            if name.startswith("wrap"):
                assert exp["wraps"] >= 1
        else:
            assert share == 0.0 and exp["se_dist"] > mg["se"], (share, exp["se_dist"])
            # noise-free: the model recovers what was sent
            sent = np.stack([m.reshape(-1) for m in c.sent["mats"]])
            assert np.array_equal(exp["sym"], sent), "the model does not recover the transmitted cells"
            assert np.array_equal(exp["pids_sym"].reshape(32, 2).T, c.sent["pids"])
    if which == "refseq":
        kind = name.split("-")[0]
        if kind.startswith("rot"):
            r, cw = int(kind[3:]), st["cfo_wait"]
            assert M.find_ref(exp["refmask"]) == r
            if cw == 0 and r > 0:
                assert er["keep"] == M.SYM + M.SYM // 2 - er["samperr"] + ((32 - r) % 32) * M.SYM and er["cfo_wait"] == 8
            else:
                assert er["keep"] == M.SYM + M.SYM // 2 - er["samperr"] and er["cfo_wait"] == (cw - 1 if cw or r else 0)
            assert (es["offset_history"] == 0x563) == (r == 0)
        elif kind.startswith("bc"):
            bc, psmi, rdbi = c.sent["bc"], c.sent["psmi"], c.sent["rdbi"]
            assert es["offset_history"] == (0x12 << 4) | bc and er["cfo_wait"] == 4
            assert (es["psmi"], es["rdbi"], es["pli"]) == ((psmi, rdbi, 0) if bc == 0 else (7, -1, -1))
        elif kind.startswith(("care", "parity")):
            assert M.find_block(exp["refmask"]) == -1 and es["offset_history"] == 0 and es["sync_state"] == M.COARSE
            assert bin(exp["refmask"] ^ sum(int(b) << n for n, b in enumerate(aa.sa.reference_bits(0)))).count("1") == 1
        elif kind == "system":
            assert (es["pli"], es["hppi"], es["aabi"], es["rdbi"], es["psmi"]) == (1, 1, 1, 0, 1) and es["offset_history"] == 0
        elif kind.startswith("hist"):
            lock = name in ("hist567-bc0", "histf567-bc0", "hist567-bc0-ma3")
            assert (es["sync_state"] == M.FINE) == lock
            if lock:
                assert er["flags"] & M.REC_TO_FINE and es["fine_epoch"] == 1 and es["am_errors"] == 0 and es["am_diversity_wait"] == 4 and es["bc"] == 1 and er["bc_decoded"] == 0
                assert es["offset_history"] == 0 and er["sis"] & 16 and er["freq_offset"] != 0.0
            else:
                assert es["offset_history"] == {"hist0567-bc3": 0x5673, "hist5670-bc0": 0x56700}[name] and es["am_errors"] == 9 and es["am_diversity_wait"] == 1
        elif kind == "fine":
            assert er["cfo_wait"] == -1
    if "cfo_ratio" in exp:
        assert exp["cfo_ratio"] >= 1.01, exp["cfo_ratio"]                      # the CFO arg-max: only inputs whose two largest sums are a percent apart
    if which == "carrier":
        if name.startswith("cfo"):
            want = float(name[3:])
            assert es["cfo"] - st["cfo"] == int(np.rint(want)), (es["cfo"], st["cfo"], want)
        if name.startswith("start"):
            assert er["samperr"] == int(name[5:]), er["samperr"]
    if which == "cells" and name.startswith("start"):
        assert er["samperr"] == int(name[5:])


def check_cover():
    """across the cells set every constellation point is sent on every carrier of every partition, and on both PIDS carriers, in both service modes"""
    for psmi in (1, 2):
        sizes = (64, 64, 64 if psmi == 2 else 16, 64 if psmi == 2 else 4)
        seen = [np.zeros((25, s), dtype=bool) for s in sizes]
        pids = np.zeros((2, 16), dtype=bool)
        for c in aa.cells():
            if c.sent["psmi"] != psmi:
                continue
            for p in range(4):
                seen[p][np.tile(np.arange(25), 32), c.sent["mats"][p].reshape(-1)] = True
            for w in range(2):
                pids[w, c.sent["pids"][w]] = True
        assert all(s.all() for s in seen) and pids.all(), psmi
    assert {c.sent["bc"] for c in aa.cells()} == set(range(8)) and {(c.sent["psmi"], c.sent["rdbi"]) for c in aa.cells()} >= {(1, 0), (1, 1), (2, 0)}
