"""`-m "not gpu"`: the band scan (nrsc5hip_scan_*, nrsc5_amd/csrc/k_scan.hip) on the CPU-emulated twin against the float64
restatement of its definition (tests/scan_model.py), and the library's host detector on model spectra of the synthetic scenes.  The
twin's "device" memory is host memory, so numpy buffers are passed by address here -- never to the real library."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import scan_model as sm

# Largest relative error of the twin's spectrum against the float64 model over the fifteen cases of test_twin_equals_float64_model
# (measured: 9.4e-13, see its docstring); the bound is 4 x that, as the margin for other seeds, and never above the hard cap.
MEASURED_REL_ERROR = 9.4e-13
REL_BOUND = 4 * MEASURED_REL_ERROR
HARD_CAP = 1e-4
assert REL_BOUND <= HARD_CAP


def _scanner(emu_lib, rate, fmt, nfft=0):
    return eng.Scanner(rate, fmt, nfft=nfft, lib_path=emu_lib)


def _push(sc, raw: np.ndarray, chunks):
    n, pos = raw.size // 2, 0
    for c in chunks:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        seg = np.ascontiguousarray(raw[2 * pos:2 * (pos + c)])
        sc.push(seg.ctypes.data, c)
        pos += c
    assert pos == n
    return sc.spectrum()[1]


@pytest.mark.parametrize("fmt", [eng.IQ_CU8, eng.IQ_CS16, eng.IQ_CF32], ids=["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("nfft", [512, 1024, 2048, 4096, 8192])
def test_twin_equals_float64_model(emu_lib, fmt, nfft):
    """Gaussian noise plus a tone 40 dB above the noise's total power, 14 segments.  Measured largest relative error over the fifteen
    cases: 9.4e-13 (a double transform on the twin against numpy float64; a float32 transform measured 1.4e-4 at nfft 8192); asserted: 4 x that, below the hard cap of 1e-4."""
    n = nfft // 2 * 15 + 37
    raw = sm.noise_plus_tone(fmt, n, seed=nfft + fmt)
    sc = _scanner(emu_lib, 2400000, fmt, nfft)
    got = _push(sc, raw, [n // 3, n - n // 3])
    assert sc.segments == sm.segments(n, nfft) >= 12
    freqs = sc.spectrum()[0]
    assert np.allclose(freqs, (np.arange(nfft) - nfft // 2) * 2400000 / nfft)
    sc.close()
    want = sm.psd(sm.scaled(raw, fmt), nfft)
    err = sm.rel_error(got, want)
    print(f"nfft {nfft} fmt {fmt}: largest relative error {err:.3e}")
    assert np.max(want) / np.median(want) > 1e4                 # the tone is there
    assert err <= REL_BOUND, err


@pytest.mark.parametrize("name", list(sm.MANY_SEGMENT_CASES))
def test_twin_many_segments_per_push(emu_lib, name):
    """More than ROWS_TARGET segments in one push: every workgroup carries its sums across a run of segments (the last run is short),
    and "rows-over-target" clamps the run to RUN_MAX with more rows than ROWS_TARGET.  Measured on the twin: 5e-14 .. 7e-14."""
    nfft, n, fmt, chunks = sm.many_segment_pushes(name)
    raw = sm.noise_plus_tone(fmt, n, seed=nfft + len(name))
    sc = _scanner(emu_lib, 2400000, fmt, nfft)
    got = _push(sc, raw, chunks)
    assert sc.segments == sm.segments(n, nfft)
    err = sm.rel_error(got, sm.psd(sm.scaled(raw, fmt), nfft))
    print(f"{name}: largest relative error {err:.3e}")
    assert err <= REL_BOUND, err
    if name == "rows-over-target":                                    # the same pushes give the same bytes: the reduce adds 1094 rows in row order
        sc.reset()
        assert _push(sc, raw, chunks).tobytes() == got.tobytes()
    sc.close()


def test_chunking_reset_and_repeatability(emu_lib):
    nfft, fmt = 512, eng.IQ_CS16
    n = nfft * 9 + 301
    raw = sm.noise_plus_tone(fmt, n, seed=5)
    rng = np.random.default_rng(6)
    plans = [[n], [7] * (n // 7 + 1), [nfft - 1] * (n // (nfft - 1) + 1), list(rng.integers(1, 1500, 200))]
    ref = None
    for chunks in plans:
        sc = _scanner(emu_lib, 2400000, fmt, nfft)
        a = _push(sc, raw, chunks)
        assert sc.segments == sm.segments(n, nfft)
        sc.reset()
        assert sc.segments == 0
        b = _push(sc, raw, chunks)                               # reset == a fresh object, and the same pushes give the same bytes
        sc.close()
        fresh = _scanner(emu_lib, 2400000, fmt, nfft)
        c = _push(fresh, raw, chunks)
        fresh.close()
        assert a.tobytes() == b.tobytes() == c.tobytes()
        if ref is None:
            ref = a
        else:
            assert sm.rel_error(a, ref) <= 1e-5
    assert sm.rel_error(ref, sm.psd(sm.scaled(raw, fmt), nfft)) <= REL_BOUND


def test_white_noise_level_and_segment_count(emu_lib):
    nfft, sigma = 512, 1500.0
    for extra in (0, 1, 255, 256, 511):
        n = nfft + 256 * 199 + extra                              # >= 200 segments
        rng = np.random.default_rng(extra)
        raw = np.clip(np.rint(sigma * rng.standard_normal(2 * n)), -32768, 32767).astype(np.int16)
        sc = _scanner(emu_lib, 1000000, eng.IQ_CS16, nfft)
        psd = _push(sc, raw, [n])
        assert sc.segments == (n - nfft) // (nfft // 2) + 1 >= 200
        sc.close()
        v = np.mean(np.abs(sm.scaled(raw, eng.IQ_CS16)) ** 2)
        assert abs(np.mean(psd) / v - 1) <= 0.02, np.mean(psd) / v
        if extra:
            break                                                 # the level once, the count for every remainder
    for extra in (1, 255, 256, 511):
        n = nfft * 3 + extra
        raw = np.zeros(2 * n, dtype=np.int16)
        sc = _scanner(emu_lib, 1000000, eng.IQ_CS16, nfft)
        sc.push(raw.ctypes.data, n)
        assert sc.segments == (n - nfft) // (nfft // 2) + 1
        sc.close()


@pytest.mark.parametrize("nfft", [512, 1024, 4096])
def test_tone_at_a_bin_centre(emu_lib, nfft):
    k = nfft // 8 + 3                                             # cycles per transform; bin index nfft/2 + k, and a negative one
    for kk in (k, -k):
        n = nfft * 4
        z = 0.4 * np.exp(2j * np.pi * kk * np.arange(n) / nfft)
        raw = np.stack([z.real, z.imag], axis=-1).reshape(-1).astype(np.float32)
        sc = _scanner(emu_lib, 2048000, eng.IQ_CF32, nfft)
        freqs, psd = (sc.push(raw.ctypes.data, n), sc.spectrum())[1]
        sc.close()
        peak = int(np.argmax(psd))
        assert peak == nfft // 2 + kk and abs(freqs[peak] - kk * 2048000 / nfft) < 1e-6
        d = np.abs(np.arange(nfft) - peak)
        far = np.minimum(d, nfft - d) > 2
        assert 10 * np.log10(np.max(psd[far]) / psd[peak]) <= -31.0


def test_default_transform_size(emu_lib):
    for rate, want in ((744187.5, 512), (1024000, 512), (1024001, 1024), (2400000, 2048), (10000000, 8192), (20000000, 8192), (64000000, 8192)):
        sc = _scanner(emu_lib, rate, eng.IQ_CS16)
        assert sc.nfft == want == sm.default_nfft(rate) and abs(sc.bin_hz - rate / want) < 1e-9
        sc.close()


def test_rejected_arguments(emu_lib):
    import ctypes

    def rejects(rate, fmt, nfft):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            _scanner(emu_lib, rate, fmt, nfft)
        assert ei.value.code == eng.EINVAL
    for nfft in (256, 16384, 1000, 3 * 512, -512, 1):
        rejects(2400000, eng.IQ_CS16, nfft)
    rejects(744187, eng.IQ_CS16, 512)
    rejects(64000001, eng.IQ_CS16, 512)
    rejects(2400000, 3, 512)
    rejects(2400000, -1, 512)
    sc = _scanner(emu_lib, 2400000, eng.IQ_CS16, 512)
    raw = np.zeros(2 * 511, dtype=np.int16)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # before any push, and before the first complete segment
        sc.spectrum()
    assert ei.value.code == eng.EINVAL
    sc.push(raw.ctypes.data, 511)
    for call in (sc.spectrum, sc.detect):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            call()
        assert ei.value.code == eng.EINVAL
    with pytest.raises(eng.Nrsc5HipError) as ei:
        sc.push(raw.ctypes.data, -1)
    assert ei.value.code == eng.EINVAL
    sc.push(raw.ctypes.data, 1)
    assert sc.segments == 1 and sc.detect() == []               # an all-zero capture: a spectrum, and nothing found
    with pytest.raises(eng.Nrsc5HipError) as ei:
        sc.detect(max_stations=-1)
    assert ei.value.code == eng.EINVAL
    sc.close()
    lib = eng.load_library(emu_lib)
    psd, n = np.ones(1024), ctypes.c_int()
    out = (eng.ScanStation * 4)()
    assert lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, 1024, 2.4e6, None, ctypes.addressof(out), -1, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, 1000, 2.4e6, None, ctypes.addressof(out), 4, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, 1024, 0.0, None, ctypes.addressof(out), 4, ctypes.byref(n)) == eng.EINVAL
    assert lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, 1024, 2.4e6, None, ctypes.addressof(out), 4, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.nrsc5hip_scan_detect_psd(psd.ctypes.data, 1024, 2.4e6, None, None, 0, ctypes.byref(n)) == 0      # NULL params: the defaults


_SCENE_CACHE = {}


def _scene_spectrum(name):
    if name not in _SCENE_CACHE:
        raw, rate, fmt, true, _ = sm.scene(name)
        raw = raw.numpy() if hasattr(raw, "numpy") else raw
        nfft = sm.default_nfft(rate)
        _SCENE_CACHE[name] = (sm.psd(sm.scaled(raw, eng.IQ_FORMATS[fmt]), nfft, max_segments=400), rate, true)
    return _SCENE_CACHE[name]


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_detector_on_model_spectra(emu_lib, name):
    psd, rate, true = _scene_spectrum(name)
    bw = rate / psd.size
    got = eng.detect_psd(psd, rate, lib_path=emu_lib)
    want = sm.detect(psd, rate)
    print(name, [(round(g["offset_hz"] / 1e3, 1), round(g["score_db"], 1)) for g in got])
    assert len(got) == len(want)                                # the library and the model agree on every pick
    for g, w in zip(got, want):
        assert round(g["offset_hz"] / bw) + psd.size // 2 == w["bin"] and abs(g["offset_hz"] - w["offset_hz"]) < 1e-6
        assert abs(g["score_db"] - np.float32(w["score_db"])) <= 1e-6 * max(1.0, abs(w["score_db"]))
        for key in ("lower_db", "upper_db", "floor_db"):
            assert abs(g[key] - w[key]) <= 1e-4
    if name == "C":                                             # no HD station: at most the slot between the two analog carriers
        assert len(got) <= 1
        assert all(abs(g["offset_hz"] - 3.0e6) > 150e3 for g in got)
        return
    assert len(got) == len(true)                                # exactly the stations
    for f in true:
        assert min(abs(g["offset_hz"] - f) for g in got) <= 1.5 * bw, (f, got)
    assert all(g["score_db"] >= 6.0 for g in got)


def test_detector_parameters(emu_lib):
    psd, rate, true = _scene_spectrum("D")
    loud = eng.detect_psd(psd, rate, threshold_db=12.0, lib_path=emu_lib)
    assert len(loud) == 3 and loud == eng.detect_psd(psd, rate, lib_path=emu_lib)[:3]
    assert len(eng.detect_psd(psd, rate, max_stations=2, lib_path=emu_lib)) == 2
    assert len(eng.detect_psd(psd, rate, min_separation_hz=2.5e6, lib_path=emu_lib)) < 4
    assert [p["bin"] for p in sm.detect(psd, rate, threshold_db=12.0)] == [round(g["offset_hz"] / (rate / psd.size)) + psd.size // 2 for g in loud]
