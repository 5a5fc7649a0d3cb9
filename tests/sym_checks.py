"""Checks of the FM symbol transform -- k_mixfft<SPW, NPAR> in its forms 1 / 2 / 4 / 8 / 16 and k_mixfft8 (form 32), bodies in csrc/mixfft_body.h -- through
nrsc5hip_stage_symbols, which runs launch_mixfft alone on caller data.  Shared by tests/test_symbol_stage_cpu.py (the CPU-emulated twin: indexing, the fold, the cut,
the parameter plumbing) and tests/test_gpu_symbol_stage.py (the gfx950 code: the same plus the inline-assembly complex products, the transcendental unit and its wait
state, the vector loads of the capture, the persistent forms' early loads).  Cases, tolerance and their derivation: tests/sym_args.py; the model: tests/sym_model.py.

 1. every bin of every symbol of every case, in every form, within the case's bound of the float64 model -- no bin excluded
 2. rows of streams that were not launched or not active still hold the fill; an active row has no slot left at the fill
 3. forms 1, 2, 4, 8, 16 leave the same bits (the same instructions on the same operands); form 32 is held to 1 alone
 4. a capture and the FIFO window holding its integer half-band leave the same bits (forms 1 and 32)
 5. (params_mode 1) launch_mixfft(local_prepare = 1) alone and launch_prepare + launch_mixfft(0) leave the same bits and read back the same parameters, and
    the bins equal the model on those parameters
 6. every tone peaks in the slot it must; a tone the cut drops (477, 745, 1303, 1571, DC) leaves every slot below 1e-3 of the in-band peak
 7. the hook refuses what it must and stays usable"""
import ctypes

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import sym_args as sa, sym_model as M

FILL = 0xA5A5A5A5
CALLS = tuple(sa.calls())


def make_engine(lib):
    return eng.Engine(max_streams=sa.MAX_STREAMS, q15_capacity=2 * 71280, lib_path=lib)


def _words(bins):
    return np.ascontiguousarray(bins, dtype=np.complex64).view(np.uint32).reshape(bins.shape + (2,))


def run_call(E, name, form):
    """one hook call -> (bins [4, 32, 534], read-back parameters), run once per engine, call and form"""
    cache = E.__dict__.setdefault("_sym_results", {})
    if (name, form) not in cache:
        call = sa.calls()[name]
        cache[(name, form)] = E.stage_symbols(form, [sa.stream_args(c) for c in call["cases"]], ids=call["ids"])
    return cache[(name, form)]


def _compare(label, got, want, bound, report=True):
    """checks 1 and 2 of one active row: got complex64 [32, 534] against the model and its per-symbol bound; -> worst error / bound"""
    w = _words(got)
    at_fill = (w == FILL).all(axis=-1)
    assert not at_fill.any(), "%s: %d slots were never written, the first in symbol %d slot %d" % (label, at_fill.sum(), *np.argwhere(at_fill)[0])
    err = np.abs(got.astype(np.complex128) - want)
    mx = np.abs(want).max(axis=1)
    worst = float((err.max(axis=1)[mx > 0] / mx[mx > 0]).max()) if (mx > 0).any() else 0.0
    ratio = float((err.max(axis=1)[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    if report:
        print("%s: worst |got - model| %.3g of the symbol's largest bin, %.3g of the bound" % (label, worst, ratio))
    bad = err > bound[:, None]
    if bad.any():
        s, k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d bins beyond the bound, the first in symbol %d slot %d (bin %d): got %r, model %r, |difference| %.4g, bound %.4g"
                             % (label, bad.sum(), s, k, M.LIVE_BINS[k], complex(got[s, k]), complex(want[s, k]), err[s, k], bound[s]))
    return ratio


def check_call(E, name, form):
    """checks 1, 2 and 6 of one call in one form, and that the parameters come back as they went in"""
    call = sa.calls()[name]
    bins, params = run_call(E, name, form)
    assert bins.shape == (sa.MAX_STREAMS, M.NSYM, M.LIVE_N)
    for s in range(sa.MAX_STREAMS):
        case = call["cases"][s] if s < len(call["cases"]) else None
        if case is None or not case["active"]:
            assert np.all(_words(bins[s]) == FILL), "%s form %d: the row of stream %d (%s) was written" % (name, form, s, "inactive" if case else "not launched")
            continue
        label = "%s form %d stream %d (%s)" % (name, form, s, case["name"])
        want, bound = sa.model(case)
        _compare(label, bins[s], want, bound)
        if case["tone_bins"] is not None:
            check_tones(label, case, np.abs(bins[s].astype(np.complex128)))
    for s, case in enumerate(call["cases"]):
        p = params[s]
        assert (p["a00"], p["theta"], p["dtheta"], p["growth"], p["active"], p["nco_mode"]) == \
               (case["a00"], case["theta"], case["dtheta"], case["growth"], case["active"], 1 if case["tab"] is not None else 0), (name, s, p)


def check_tones(label, case, mag):
    """check 6 on |bins| [32, 534] of a tone case (the device's, or the model's own)"""
    slots = np.array([M.slot_of(b) for b in case["tone_bins"]])
    peak = mag[slots >= 0, :].max()
    assert peak > 0.9 * case["amp"] * M.FFT_N / 32767.0, (label, peak)
    for i, k in enumerate(slots):
        if k >= 0:
            assert int(mag[i].argmax()) == k, "%s: symbol %d peaks in slot %d, its tone belongs in slot %d (bin %d)" % (label, i, mag[i].argmax(), k, case["tone_bins"][i])
        else:
            assert mag[i].max() < 1e-3 * peak, "%s: symbol %d's tone at bin %d is outside the cut and left %.3g of the in-band peak" % (label, i, case["tone_bins"][i], mag[i].max() / peak)


def check_forms(E, name):
    """check 3"""
    ref = _words(run_call(E, name, 1)[0])
    for form in (2, 4, 8, 16):
        got = _words(run_call(E, name, form)[0])
        diff = (got != ref).any(axis=-1)
        assert not diff.any(), "%s: form %d differs from form 1 in %d bins, the first in stream %d symbol %d slot %d" % (name, form, diff.sum(), *np.argwhere(diff)[0])


def check_raw_equals_fifo(E, form):
    """check 4: every capture case beside the FIFO window that holds its half-band"""
    n = 0
    for call in sa.calls().values():
        if call["ids"] is not None:
            continue
        for case in call["cases"]:
            if case["kind"] != "raw" or not case["active"]:
                continue
            bins, _ = E.stage_symbols(form, [sa.stream_args(case), sa.stream_args(case, kind="fifo")])
            a, b = _words(bins[0]), _words(bins[1])
            diff = (a != b).any(axis=-1)
            assert not diff.any(), "form %d, %s: capture and FIFO differ in %d bins, the first in symbol %d slot %d: %r / %r" % \
                (form, case["name"], diff.sum(), *np.argwhere(diff)[0], complex(bins[0][tuple(np.argwhere(diff)[0])]), complex(bins[1][tuple(np.argwhere(diff)[0])]))
            n += 1
    assert n >= 12
    return n


def check_prepare(E, form):
    """check 5"""
    streams, cases = sa.prepare_streams()
    fused, pf = E.stage_symbols(form, streams, params_mode=1, prepare=1)
    split, ps = E.stage_symbols(form, streams, params_mode=1, prepare=0)
    assert pf == ps, (pf, ps)
    assert np.array_equal(_words(fused), _words(split)), "form %d: local_prepare = 1 and launch_prepare + local_prepare = 0 leave different bins" % form
    assert np.all(_words(fused[len(streams):]) == FILL)
    for s, (st, case) in enumerate(zip(streams, cases)):
        p = pf[s]
        assert p["active"] == 1 and p["nco_mode"] == 0 and p["a00"] == st["rd"] + 1080 + st["samperr"], p
        # acquire.c:112-168 in float64: the angle, the per-sample step (within the float32 rounding of angle / 2048 and of its sine and cosine) and the start phase
        angle = (st["prev_angle"] - st["angle"]) - 2 * np.pi * st["cfo"]
        assert abs(p["dtheta"] - angle / 2048) <= 2e-7 * max(1.0, abs(angle)) and abs(p["growth"]) <= 1.2e-7, p
        th = st["theta"] - (1080 - (1080 + st["samperr"])) * angle / 2048
        assert abs(np.angle(np.exp(1j * (p["theta"] - th)))) <= 1e-6, (p, th)
        want, bound = sa.model(case, params=p)
        _compare("prepare form %d stream %d (%s)" % (form, s, case["name"]), fused[s], want, bound)


def check_rejections(E):
    """check 7: every request the hook must refuse (NRSC5HIP_EINVAL, nothing launched), each followed by a valid call that passes check 1"""
    call = sa.calls()["noise fifo"]
    good = [sa.stream_args(c) for c in call["cases"]]
    raw_case = sa.calls()["noise raw"]["cases"][0]

    def refused(form, streams, **kw):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            E.stage_symbols(form, streams, **kw)
        assert ("error %d:" % eng.EINVAL) in str(ei.value), str(ei.value)
        bins, _ = E.stage_symbols(1, good)
        for s, c in enumerate(call["cases"]):
            _compare("after a refusal, stream %d" % s, bins[s], *sa.model(c), report=False)

    def changed(d, **kw):
        d = dict(d); d.update(kw)
        return d

    for form in (0, 3, 5, 64, -1, 100):
        refused(form, good)
    refused(1, good, n=0)
    refused(1, good, n=-1)
    refused(1, [good[0]] * (sa.MAX_STREAMS + 1))
    refused(1, None, n=1)                                                           # null stream array
    one = (eng.abi.SymStream * 1)()
    one[0].q15, one[0].q15_samples, one[0].active = good[0]["q15"].ctypes.data, sa.BLOCK, 1
    room, back = np.zeros((sa.MAX_STREAMS, M.NSYM, M.LIVE_N), dtype=np.complex64), (eng.abi.SymParams * 1)()
    for bins_p, out_p in ((None, ctypes.addressof(back)), (room.ctypes.data, None)):  # null outputs
        rc = E.lib.nrsc5hip_stage_symbols(E._h, 1, 1, 0, 0, ctypes.addressof(one), None, bins_p, out_p)
        assert rc == eng.EINVAL, rc
    assert E.lib.nrsc5hip_stage_symbols(E._h, 1, 1, 0, 0, ctypes.addressof(one), None, room.ctypes.data, ctypes.addressof(back)) == 0
    _compare("after null outputs", room[0], *sa.model(call["cases"][0]), report=False)
    refused(1, [changed(good[0], q15=None)])                                        # neither samples
    refused(1, [changed(sa.stream_args(raw_case), q15=sa.q15(raw_case))])           # both
    refused(1, good, params_mode=2)
    refused(1, good, params_mode=1, prepare=2)
    refused(1, good, ids=(0, 0))
    refused(1, good, ids=(0, 2))
    refused(1, [changed(good[0], a00=-1)])
    refused(1, [changed(good[0], a00=1)])                                           # the last symbol's last sample lies one beyond the window
    refused(1, [changed(good[0], q15_samples=sa.BLOCK - 1)])
    refused(1, [changed(good[0], a00=1 << 62)])
    raw = sa.stream_args(raw_case)
    dwords = raw_case["samples"].size // 4
    refused(1, [changed(raw, a00=dwords - sa.BLOCK + 1)])                           # ... beyond the capture
    refused(1, [changed(raw, raw_bytes=raw_case["samples"].size - 4, a00=dwords - sa.BLOCK)])
    refused(1, [changed(raw, raw_bytes=raw_case["samples"].size - 1)])
    for lead in (-4, 1, 2, 16):
        refused(1, [changed(raw, lead=lead)])
    refused(1, [changed(good[0], nco_mode=1)])                                      # exact mode without a table
    streams, _ = sa.prepare_streams()
    refused(1, [changed(streams[0], wr=streams[0]["wr"] - 1)], params_mode=1)       # a sample short of a window
    refused(1, [changed(streams[0], wr=streams[0]["wr"] + 1)], params_mode=1)       # beyond the samples given
    refused(1, [changed(streams[0], rd=-1)], params_mode=1)
    refused(1, [changed(streams[0], samperr=1081)], params_mode=1)
    assert E.stage_symbols(1, [changed(raw, a00=dwords - sa.BLOCK)])[0].shape[0] == sa.MAX_STREAMS      # ends on the capture's last dword: taken


# ---- the inputs themselves (no device) ----------------------------------------------------------------------------------------------------------------------
def _all_cases():
    seen = {}
    for call in sa.calls().values():
        for c in call["cases"]:
            seen.setdefault(c["name"], c)
    return list(seen.values())


def dropped_symbols(case):
    """symbols of a tone case whose tone the cut drops: their live bins hold nothing but the residue of rounding the samples to integers"""
    if case["tone_bins"] is None:
        return np.zeros(M.NSYM, dtype=bool)
    return np.array([M.slot_of(b) < 0 for b in case["tone_bins"]])


def check_reference_arithmetic(oracle):
    """the reference's float32 arithmetic against the float64 model, relative to the symbol's largest live bin, over every case -> the largest figure.  Symbols
    whose tone the cut drops are measured against the case's in-band peak: their own largest live bin is 1e-7 of the tone the arithmetic is busy with."""
    worst = 0.0
    for c in _all_cases():
        want, _ = sa.model(c)
        ref = M.reference32(oracle, sa.q15(c), c["a00"], sa.phasors(c))
        err, mx = np.abs(ref - want).max(axis=1), np.abs(want).max(axis=1)
        drop = dropped_symbols(c)
        if drop.any():
            mx = np.where(drop, mx[~drop].max(), mx)
        assert np.all(err[mx == 0] == 0), c["name"]
        rel = float((err[mx > 0] / mx[mx > 0]).max())
        print("%-50s reference arithmetic: %.3g of the largest bin" % (c["name"], rel))
        worst = max(worst, rel)
    print("worst: %.3g (SYM_ERR_MEASURED %.3g)" % (worst, sa.SYM_ERR_MEASURED))
    assert worst <= sa.SYM_ERR_MEASURED, worst
    assert worst >= 0.5 * sa.SYM_ERR_MEASURED, "SYM_ERR_MEASURED is no longer the measured figure rounded up: %.3g" % worst
    return worst


def check_bounds_are_tight():
    """no symbol's bound exceeds 1e-4 of its largest bin (a symbol whose tone the cut drops: of the case's in-band peak)"""
    for c in _all_cases():
        want, bound = sa.model(c)
        mx = np.abs(want).max(axis=1)
        drop = dropped_symbols(c)
        if drop.any():
            mx = np.where(drop, mx[~drop].max(), mx)
        assert np.all(bound[mx == 0] == 0), c["name"]
        assert np.all(bound <= 1e-4 * mx), "%s: bound %.3g of the largest bin" % (c["name"], (bound[mx > 0] / mx[mx > 0]).max())
    _, cases = sa.prepare_streams()
    assert len(cases) == 3


def check_tone_cases():
    """every tone case's expected slot is the model's arg-max, a dropped tone leaves the model's live bins below 1e-3 of the peak; every edge bin, both sides of it, DC
    and every shift occur"""
    bins, shifts = set(), set()
    for c in _all_cases():
        if c["tone_bins"] is None:
            continue
        check_tones("model of " + c["name"], c, np.abs(sa.model(c)[0]))
        bins.update(c["tone_bins"]); shifts.add(int(round(c["dtheta"] * M.FFT_N / (2 * np.pi))))
    assert bins == set(sa.BINS_ALL) and shifts == {0} | set(sa.SHIFTS)
