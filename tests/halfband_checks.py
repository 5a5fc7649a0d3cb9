"""Checks of the fused float32 half-band (csrc/halfband_raw.h) through nrsc5hip_stage_halfband_raw, shared by
tests/test_halfband_stage_cpu.py (the CPU-emulated twin: indexing, unpacking, the stream-start branch) and tests/test_gpu_halfband_stage.py
(the gfx950 code: the same plus the inline assembly and the rounding-mode switch).  The stage kernels call the production functions of
all three device forms -- hb_sample_q15, raw_symbol_load + raw_symbol_halfband, raw_symbol_load8 + raw_symbol_halfband8 -- and

* every output must EQUAL oracle.halfband_fm_cu8 (the C restatement of firdecim_q15.c, zero history) on every set and request of
  tests/halfband_args.py: no tolerance;
* the three forms must equal each other (implied, asserted on its own because it says which form is the odd one out);
* the rounding probe and the denormal probe every work-item of the symbol forms evaluates in front of the half-band and behind it must
  show round-to-nearest and a kept denormal."""
import functools

import numpy as np

from nrsc5_amd import engine as eng
from tests import halfband_args as ha

FORMS = ((eng.HB_ACQ, "HB_ACQ"), (eng.HB_SYM128, "HB_SYM128"), (eng.HB_SYM256, "HB_SYM256"))
PROBE_NEAREST = 0x3f800001                # 1.0f + 1.5 * 2^-24 rounded to nearest (0x3f800000 when rounding down)
PROBE_DENORMAL = 0x00200000               # 2^-126 * 0.5f kept (0 when flushed)
_ORACLE = None


def make_engine(lib):
    return eng.Engine(max_streams=1, q15_capacity=2 * 71280, lib_path=lib)


@functools.lru_cache(maxsize=None)
def _reference(name):
    exp, _ = _ORACLE.halfband_fm_cu8(ha.get(name))
    exp.setflags(write=False)
    return exp


def reference(oracle, name):
    """the integer code's outputs for a whole set, computed once per set and session: int16 [dwords, 2]"""
    global _ORACLE
    _ORACLE = oracle
    return _reference(name)


def run_form(E, form, name, lead):
    """-> {(a0, symbols): (outputs, probes or None)} of one set in one form at one placement; HB_ACQ produces the same samples one by one"""
    out = {}
    for a0, n in ha.requests(name):
        if form == eng.HB_ACQ:
            out[(a0, n)] = (E.stage_halfband_raw(form, ha.get(name), a0, n * ha.SYM_N, lead=lead), None)
        else:
            out[(a0, n)] = E.stage_halfband_raw(form, ha.get(name), a0, n, lead=lead, probe=True)
    return out


def _where(form, j):
    """work-item and slot that produced output j of a symbol"""
    j %= ha.SYM_N
    if form == eng.HB_SYM128:
        return "work-item %d output %d" % (j // 17, j % 17)
    if form == eng.HB_SYM256:
        return "work-item %d output %d" % (j // 9, j % 9)
    return "lane %d" % (j % 256)


def _mismatch_lines(form, fname, name, lead, a0, got, exp, limit=6):
    bad = np.flatnonzero((got != exp).any(axis=1))
    lines = ["%s set %s lead %d a0 %d: %d of %d outputs differ" % (fname, name, lead, a0, bad.size, got.shape[0])]
    for j in bad[:limit]:
        lines.append("    sample %d (%s): got (%d, %d) expected (%d, %d)" % (a0 + j, _where(form, j), got[j, 0], got[j, 1], exp[j, 0], exp[j, 1]))
    return lines


def check_set(E, oracle, name, report=None):
    """one set through all three forms at every lead: forms equal to each other and to the integer code, probes as in round-to-nearest.
    -> outputs compared per form.  report: a list that receives one line per form (and the mismatches, if any)"""
    exp = reference(oracle, name)
    compared = {fname: 0 for _, fname in FORMS}
    wrong = {fname: 0 for _, fname in FORMS}
    lines, disagree, probes_seen, probe_bad = [], [], set(), []
    for lead in ha.LEADS:
        res = {fname: run_form(E, form, name, lead) for form, fname in FORMS}
        for key in res["HB_ACQ"]:
            a0, n = key
            for form, fname in FORMS:
                got, pr = res[fname][key]
                want = exp[a0:a0 + n * ha.SYM_N]
                assert got.shape == want.shape
                compared[fname] += got.shape[0]
                nbad = int((got != want).any(axis=1).sum())
                if nbad:
                    wrong[fname] += nbad
                    if len(lines) < 40:
                        lines += _mismatch_lines(form, fname, name, lead, a0, got, want)
                if pr is not None:
                    probes_seen.update(map(tuple, np.unique(pr.reshape(-1, 4), axis=0).tolist()))
                    ok = (pr[..., 0] == PROBE_NEAREST) & (pr[..., 2] == PROBE_NEAREST) & (pr[..., 1] != 0) & (pr[..., 3] != 0)
                    if not ok.all() and len(probe_bad) < 8:
                        s, w = np.argwhere(~ok)[0]
                        probe_bad.append("%s set %s lead %d a0 %d symbol %d work-item %d: rounding 0x%08x / 0x%08x, denormal 0x%08x / 0x%08x (before / behind)"
                                         % (fname, name, lead, a0, s, w, pr[s, w, 0], pr[s, w, 2], pr[s, w, 1], pr[s, w, 3]))
            for (fa, na), (fb, nb) in ((FORMS[0], FORMS[1]), (FORMS[0], FORMS[2]), (FORMS[1], FORMS[2])):
                if not np.array_equal(res[na][key][0], res[nb][key][0]):
                    disagree.append("%s != %s: set %s lead %d a0 %d" % (na, nb, name, lead, a0))
    if report is not None:
        for _, fname in FORMS:
            report.append("%-10s %-13s %8d outputs compared, %s" % (fname, name, compared[fname], "all equal" if not wrong[fname] else "%d DIFFER" % wrong[fname]))
        report.extend(lines)
        report.append("%-10s %-13s probes (rounding before, denormal before, rounding behind, denormal behind): %s"
                      % ("", name, "; ".join(" ".join("0x%08x" % v for v in p) for p in sorted(probes_seen))))
    assert not disagree, "the forms differ among themselves:\n" + "\n".join(disagree[:12]) + "\nagainst the integer code: " + repr(wrong) + "\n" + "\n".join(lines[:14])
    assert not any(wrong.values()), "outputs differ from the integer code " + repr(wrong) + ":\n" + "\n".join(lines)
    assert not probe_bad, "rounding mode or denormal handling not as the kernel was entered with:\n" + "\n".join(probe_bad)
    return compared


def check_acq_span(E, oracle, n=700):
    """HB_ACQ over one contiguous span from sample 0 on: history in the first seven samples, and the step from one 256-lane workgroup to
    the next (twice), at every lead"""
    exp = reference(oracle, "uniform")[:n]
    for lead in ha.LEADS:
        got = E.stage_halfband_raw(eng.HB_ACQ, ha.get("uniform"), 0, n, lead=lead)
        assert np.array_equal(got, exp), "\n".join(_mismatch_lines(eng.HB_ACQ, "HB_ACQ", "uniform", lead, 0, got, exp))
    one = E.stage_halfband_raw(eng.HB_ACQ, ha.get("uniform"), 255, 2)          # the boundary alone: last lane of a workgroup, and a request of two
    assert np.array_equal(one, reference(oracle, "uniform")[255:257])
    return n


def check_rejections(E):
    """every request the hook must refuse (NRSC5HIP_EINVAL, nothing launched), and the largest ones it must take"""
    import pytest
    iq = ha.get("const0")
    d = iq.size // 4

    def refused(form, data, a0, n, lead=0, nbytes=None):
        out = np.zeros((4 * ha.SYM_N, 2), dtype=np.int16)
        with pytest.raises(eng.Nrsc5HipError) as ei:
            E._check(E.lib.nrsc5hip_stage_halfband_raw(E._h, form, data.ctypes.data, data.size if nbytes is None else nbytes, lead, a0, n, out.ctypes.data, None))
        assert ("error %d:" % eng.EINVAL) in str(ei.value), str(ei.value)

    for form in (-1, 3, 32):
        refused(form, iq, 0, 1)
    for form, _ in FORMS:
        for lead in (-4, 1, 2, 6, 16):
            refused(form, iq, 7, 1, lead=lead)
        refused(form, iq, 7, 0)
        refused(form, iq, 7, -1)
        refused(form, iq, -1, 1)
        for nbytes in (iq.size - 1, iq.size - 2, iq.size - 3):
            refused(form, iq, 7, 1, nbytes=nbytes)
        per = 1 if form == eng.HB_ACQ else ha.SYM_N
        last = d - per
        assert E.stage_halfband_raw(form, iq, last, 1).shape == (per, 2)                 # ends on the last dword: taken
        refused(form, iq, last + 1, 1)                                                    # one sample beyond it
        refused(form, iq, d + 5, 1)
        refused(form, iq, 0, d // per + 1)
        refused(form, iq, 1 << 62, 1)
        refused(form, iq, 0, 1 << 62)
        refused(form, iq, last, 1, nbytes=iq.size - 4)                                    # the same request on a capture one dword shorter
