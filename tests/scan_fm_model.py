"""Restatement of the analog-carrier detector (nrsc5hip_scan_detect_fm_psd, include/nrsc5hip.h "band scan") in numpy, and the hand-made spectra
tests/test_scan_fm_cpu.py runs it on."""
import numpy as np

from tests import scan_model as sm

SCORE_HZ, CENTROID_HZ = 50e3, 100e3
FS, NFFT = 2400000.0, 2048


def detect_fm(p: np.ndarray, fs: float, threshold_db: float = 6.0, min_separation_hz: float = 150e3) -> list:
    """-> [{"bin", "bin_hz", "offset_hz", "score_db", "floor_db"}, ...], highest score first"""
    nfft = p.size
    bw = fs / nfft
    floor_p = np.sort(p)[int(sm.FLOOR_QUANTILE * (nfft - 1))]
    if not floor_p > 0:
        return []
    pre = np.concatenate([[0.0], np.cumsum(p)])
    pp = np.concatenate([p, [0.0]])

    def integral(f):
        x = np.clip(f / bw + nfft // 2 + 0.5, 0, nfft)
        k = np.floor(x).astype(np.int64)
        return pre[k] + (x - k) * pp[k], x

    c = (np.arange(nfft) - nfft // 2) * bw
    (i0, x0), (i1, x1) = integral(c - SCORE_HZ), integral(c + SCORE_HZ)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = 10 * np.log10((i1 - i0) / (x1 - x0) / floor_p)
    ok = np.abs(c) <= fs / 2 - sm.EDGE_HZ
    cand = [i for i in range(nfft) if ok[i] and np.isfinite(score[i]) and score[i] >= threshold_db]
    cand.sort(key=lambda i: (-score[i], i))
    picks = []
    for i in cand:
        if any(abs(c[i] - q["bin_hz"]) <= min_separation_hz for q in picks):
            continue
        sw = sfw = 0.0
        for k in range(nfft):                                   # in bin order, as the library adds them
            if abs(c[k] - c[i]) <= CENTROID_HZ:
                w = p[k] - floor_p if p[k] > floor_p else 0.0
                sw += w
                sfw += c[k] * w
        picks.append({"bin": i, "bin_hz": float(c[i]), "offset_hz": float(sfw / sw if sw > 0 else c[i]), "score_db": float(score[i]),
                      "floor_db": float(10 * np.log10(floor_p))})
    return picks


def freqs(nfft: int = NFFT, fs: float = FS) -> np.ndarray:
    return (np.arange(nfft) - nfft // 2) * fs / nfft


def carrier(f: np.ndarray, centre: float, power_db: float, width: float = 60e3) -> np.ndarray:
    """the spectrum of a modulated FM carrier, roughly: a raised cosine `width` wide on either side of the centre, peak power_db over 1"""
    u = np.clip(np.abs(f - centre) / width, 0, 1)
    return 10 ** (power_db / 10) * 0.5 * (1 + np.cos(np.pi * u)) * (u < 1)


def hybrid(f: np.ndarray, centre: float, host_db: float, sb_db: float) -> np.ndarray:
    """a hybrid station: the host and two flat digital sidebands at 129 361 .. 198 402 Hz"""
    a = np.abs(f - centre)
    return carrier(f, centre, host_db) + 10 ** (sb_db / 10) * ((a >= sm.SB_LO_HZ) & (a <= sm.SB_HI_HZ))


def spectra() -> dict:
    """name -> (psd, fs, the true centres in Hz that must be found, in any order; None: compare with the model only)"""
    f = freqs()
    bw = FS / NFFT
    flat = np.ones(NFFT)
    rng = np.random.default_rng(50)
    rough = flat * (1 + 0.05 * rng.standard_normal(NFFT))
    edge = FS / 2 - sm.EDGE_HZ
    last = np.floor(edge / bw) * bw                             # the outermost bin centre the channelizer can tune
    return {
        "on_a_bin": (rough + carrier(f, 100 * bw, 30), FS, [100 * bw]),
        "between_bins": (rough + carrier(f, 100.5 * bw, 30), FS, [100.5 * bw]),
        "off_by_a_third": (rough + carrier(f, -300.33 * bw, 25), FS, [-300.33 * bw]),
        "neighbours_30db": (rough + carrier(f, -100e3, 40) + carrier(f, 100e3, 10), FS, [-100e3, 100e3]),
        "hybrid": (rough + hybrid(f, 0.0, 35, 12), FS, None),
        "empty": (np.zeros(NFFT), FS, []),
        "flat": (flat, FS, []),
        "edges": (rough + carrier(f, last, 30) + carrier(f, -last, 30) + carrier(f, last + 150e3, 40), FS, None),
        "ties": (ties(), 2048000.0, None),
    }


def ties() -> np.ndarray:
    """at 2.048 MS/s and 2048 bins (1 kHz each) the score window is 100 bins and two half bins, and with integer powers every sum is exact: two
    equal rectangular carriers 61 bins wide give the same score to both and to every centre whose window holds a whole one -- the lower bin wins"""
    p = np.ones(2048)
    for centre in (-300, 300):
        p[1024 + centre - 30:1024 + centre + 31] += 64.0
    return p
