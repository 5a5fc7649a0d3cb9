"""`-m "not gpu"`: the detector of analog FM carriers (nrsc5hip_scan_detect_fm_psd: host code, no device) against its restatement
tests/scan_fm_model.py on hand-made spectra."""
import ctypes

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import scan_fm_model as sfm, scan_model as sm

SPECTRA = sfm.spectra()


def _same(got: list, want: list):
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g["bin_hz"] == w["bin_hz"], (g, w)                                # the same picks in the same order
        assert abs(g["offset_hz"] - w["offset_hz"]) <= 1e-6 and abs(g["score_db"] - w["score_db"]) <= 1e-4 and abs(g["floor_db"] - w["floor_db"]) <= 1e-4, (g, w)


@pytest.mark.parametrize("name", list(SPECTRA))
def test_detector_equals_the_model(emu_lib, name):
    psd, fs, centres = SPECTRA[name]
    got = eng.detect_fm_psd(psd, fs, lib_path=emu_lib)
    want = sfm.detect_fm(psd, fs)
    _same(got, want)
    if centres is not None:
        assert len(got) == len(centres), got
        for c in centres:                                                       # the centroid finds the carrier, on a bin or between two
            assert min(abs(g["offset_hz"] - c) for g in got) <= 0.1 * fs / psd.size, (c, got)


def test_weak_neighbour_on_the_raster_is_found_behind_a_strong_one(emu_lib):
    psd, fs, _ = SPECTRA["neighbours_30db"]
    got = eng.detect_fm_psd(psd, fs, lib_path=emu_lib)
    assert [round(g["offset_hz"] / 1e3) for g in got] == [-100, 100] and got[0]["score_db"] - got[1]["score_db"] > 25.0
    # with a separation under the raster the strong carrier's shoulder is picked as well
    assert len(eng.detect_fm_psd(psd, fs, min_separation_hz=60e3, lib_path=emu_lib)) > 2


def test_hybrid_sidebands_are_nominated_too(emu_lib):
    psd, fs, _ = SPECTRA["hybrid"]
    got = eng.detect_fm_psd(psd, fs, lib_path=emu_lib)
    at = sorted(g["offset_hz"] for g in got)
    assert len(at) == 3 and abs(at[1]) < 600.0                                  # the host ...
    mid = 0.5 * (sm.SB_LO_HZ + sm.SB_HI_HZ)
    assert abs(at[0] + mid) < 20e3 and abs(at[2] - mid) < 20e3                  # ... and both sidebands: generous on purpose


def test_edge_limit(emu_lib):
    psd, fs, _ = SPECTRA["edges"]
    got = eng.detect_fm_psd(psd, fs, lib_path=emu_lib)
    edge = fs / 2 - sm.EDGE_HZ
    assert len(got) >= 2 and all(abs(g["bin_hz"]) <= edge for g in got)         # the carrier beyond the limit is never picked as a centre
    bw = fs / psd.size
    assert {round(g["bin_hz"] / bw) for g in got} >= {int(edge // bw), -int(edge // bw)}


def test_exact_ties_go_to_the_lower_bin(emu_lib):
    psd, fs, _ = SPECTRA["ties"]
    got = eng.detect_fm_psd(psd, fs, lib_path=emu_lib)
    # the window of centre i is half of bin i - 50, bins i - 49 .. i + 49 and half of bin i + 50: it holds a whole carrier (bins c - 30 .. c + 30)
    # for i = c - 19 .. c + 19, and these all tie: the lowest of the lower carrier wins, then the lowest of the upper one
    assert [g["bin_hz"] for g in got] == [-319e3, 281e3] and got[0]["score_db"] == got[1]["score_db"]
    assert [g["offset_hz"] for g in got] == [-300e3, 300e3]                      # the centroid is the carrier all the same


def test_parameters_and_rejected_arguments(emu_lib):
    psd, fs, _ = SPECTRA["neighbours_30db"]
    assert len(eng.detect_fm_psd(psd, fs, threshold_db=30.0, lib_path=emu_lib)) == 1
    assert len(eng.detect_fm_psd(psd, fs, max_stations=1, lib_path=emu_lib)) == 1
    lib = eng.load_library(emu_lib)
    out = (eng.ScanFmStation * 4)()
    n = ctypes.c_int()
    p = np.ascontiguousarray(psd)
    assert lib.nrsc5hip_scan_detect_fm_psd(p.ctypes.data, 2048, fs, None, ctypes.addressof(out), -1, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_fm_psd(p.ctypes.data, 2000, fs, None, ctypes.addressof(out), 4, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_fm_psd(p.ctypes.data, 2048, 0.0, None, ctypes.addressof(out), 4, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_fm_psd(None, 2048, fs, None, ctypes.addressof(out), 4, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_fm_psd(p.ctypes.data, 2048, fs, None, None, 0, ctypes.byref(n)) == 0 and n.value == 2     # NULL params: the defaults


def test_scanner_object_runs_the_same_detector(emu_lib):
    rng = np.random.default_rng(3)
    n, rate = 400000, 2400000
    t = np.arange(n) / rate
    x = 300.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 8000.0 * np.exp(1j * (2 * np.pi * 250e3 * t + 3.0 * np.sin(2 * np.pi * 15e3 * t)))
    raw = np.empty(2 * n, dtype=np.int16)
    raw[0::2], raw[1::2] = np.rint(x.real), np.rint(x.imag)
    sc = eng.Scanner(rate, eng.IQ_CS16, lib_path=emu_lib)
    sc.push(raw.ctypes.data, n)
    _, psd = sc.spectrum()
    got = sc.detect_fm()
    sc.close()
    _same(got, sfm.detect_fm(psd, float(rate)))
    assert len(got) == 1 and abs(got[0]["offset_hz"] - 250e3) < 1000.0
