"""Float64 restatement of the reception impairments' definition (include/nrsc5hip.h "reception impairments"), in numpy, on top of
tests/fm_model.py and tests/carrier_model.py: what nrsc5hip_fm_impair* is checked against.  dtype=np.float32 runs the channel filter, the
envelope, the discriminator, the amplitude e and the two band-pass filters in float32 (the block sums stay double, as the definition has them):
the reference's own estimate of how far a float32 implementation may sit from the float64 one.  The sums with a stated order (block, windowed,
running) and the figures are restated operation by operation, so that they can be compared bit for bit."""
import math

import numpy as np

from tests import carrier_model as cm, fm_model as fm

BLOCK, W = fm.BLOCK, fm.W
UT, NS = 63, 11                                # NRSC5HIP_FM_IMPAIR_TAPS / _NSUMS
EDGE_LO, EDGE_HI, BETA = 100e3, 170e3, 8.0
MOD_MIN = 1e-6                                 # NRSC5HIP_FM_IMPAIR_MOD_MIN
DB_MIN, DB_MAX = cm.DB_MIN, cm.DB_MAX
SUMS = ("sx", "sxx", "sxxx", "sxxxx", "sy", "sxy", "sxxy", "syy", "cee", "cdd", "ced")
FIGURES = ("explained", "depth", "slope", "curvature", "usn_db", "ripple_db", "rho")
DEFAULTS = dict(explained_min=0.5, depth_min=0.05, rho_min=0.5)


def design_hu() -> np.ndarray:
    """63 taps, float64: the Kaiser-windowed (beta 8) difference of two sincs with edges 100 kHz and 170 kHz at Fs1, symmetric about tap 31"""
    tau = np.arange(UT, dtype=np.float64) - (UT - 1) / 2
    u = 2 * tau / (UT - 1)
    w = np.i0(BETA * np.sqrt(np.clip(1 - u * u, 0, None))) / np.i0(BETA)
    f1, f2 = EDGE_LO / fm.FS1, EDGE_HI / fm.FS1
    return (2 * f2 * np.sinc(2 * f2 * tau) - 2 * f1 * np.sinc(2 * f1 * tau)) * w


def amplitude(r: np.ndarray, dtype=np.float64) -> np.ndarray:
    """e[m] = sqrt(r[m] r[m - 1]), e[0] = 0; in float32 the product is rounded, then the correctly rounded root"""
    r = r.astype(dtype)
    e = np.sqrt((r * np.concatenate([np.zeros(1, dtype), r[:-1]])).astype(dtype)).astype(dtype)
    if e.size:
        e[0] = 0
    return e


def bandpass(v: np.ndarray, hu: np.ndarray, dtype=np.float64) -> np.ndarray:
    """sum_i hU[i] v[m - i], one chain per output, i ascending, samples in front of the stream zero.  In float32 every step is rounded once from
    the double sum of the exact product and the accumulator: an fma but for the rare double rounding"""
    h = np.asarray(hu, dtype=np.float32).astype(np.float64)
    vp = np.concatenate([np.zeros(UT - 1, np.float64), v.astype(np.float64)])
    at = np.arange(v.size, dtype=np.int64) + (UT - 1)
    acc = np.zeros(v.size, dtype)
    for i in range(UT):
        acc = (acc.astype(np.float64) + h[i] * vp[at - i]).astype(dtype)
    return acc


def terms(d: np.ndarray, e: np.ndarray, eu: np.ndarray, du: np.ndarray) -> np.ndarray:
    """the eleven summands per sample, float64 [NS][n], each product formed as the definition states it"""
    x, y, u, v = (a.astype(np.float64) for a in (d, e, eu, du))
    x2 = x * x
    return np.stack([x, x2, x2 * x, x2 * x2, y, x * y, x2 * y, y * y, u * u, v * v, u * v])


def front(x: np.ndarray, ha: np.ndarray, hu: np.ndarray, dtype=np.float64) -> dict:
    """x int16 [n, 2] -> {"r", "d", "e", "eu", "du" (dtype, [ceil(n / 2)]), "t": block sums float64 [complete blocks][NS] (numpy's sum)}"""
    r, d, _ = cm.front(x, ha, dtype)
    e = amplitude(r, dtype)
    eu, du = bandpass(e, hu, dtype), bandpass(d, hu, dtype)
    nb = r.size // BLOCK
    s = terms(d[:nb * BLOCK], e[:nb * BLOCK], eu[:nb * BLOCK], du[:nb * BLOCK])
    t = s.reshape(NS, nb, BLOCK).sum(axis=2).T.copy() if nb else np.zeros((0, NS))
    return {"r": r, "d": d, "e": e, "eu": eu, "du": du, "t": t}


def block_sums_in_order(d: np.ndarray, e: np.ndarray, eu: np.ndarray, du: np.ndarray) -> np.ndarray:
    """the block records of given float32 d, e, eu, du in the definition's order (lane l takes l + 64 i, i ascending, then the butterfly)"""
    nb = d.size // BLOCK
    s = terms(d[:nb * BLOCK], e[:nb * BLOCK], eu[:nb * BLOCK], du[:nb * BLOCK]).reshape(NS, nb, BLOCK)
    out = np.zeros((nb, NS))
    idx = np.arange(64)
    for q in range(NS):
        lanes = np.zeros((nb, 64))
        for i in range((BLOCK + 63) // 64):
            n = min(64, BLOCK - 64 * i)
            lanes[:, :n] += s[q, :, 64 * i:64 * i + n]
        for step in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ step]
        out[:, q] = lanes[:, 0]
    return out


def windowed(t: np.ndarray, ja: int):
    """the windowed sums of audio block ja from the block records t [blocks][NS] (blocks > ja + W) -> ([NS], count)"""
    win = cm.window32()
    out = []
    for q in range(NS):
        lanes = np.zeros(64)
        for lane in range(2 * W + 1):
            jb = ja + lane - W
            if jb >= 0:
                lanes[lane] = t[jb, q] * win[lane]
        out.append(cm.butterfly(lanes))
    count = 0.0
    for w in win:
        count += float(w)
    return out, count


def running(t: np.ndarray, blocks: int):
    s = [0.0] * NS
    for j in range(blocks):
        for q in range(NS):
            s[q] = s[q] + float(t[j, q])
    return s, float(blocks)


def _clamp_db(v: float) -> float:
    return DB_MIN if not v >= DB_MIN else DB_MAX if v > DB_MAX else v


def figures(sums, count: float, cfg=None) -> dict:
    """the figures and the verdict of a set of sums, line by line as include/nrsc5hip.h states them (Python floats are IEEE doubles)"""
    cfg = {**DEFAULTS, **(cfg or {})}
    out = {k: 0.0 for k in FIGURES}
    out.update(multipath=False, adjacent=False, side=0)
    if not count > 0:
        return out
    sx, sxx, sxxx, sxxxx, sy, sxy, sxxy, syy, cee, cdd, ced = (float(v) for v in sums)
    n = 540.0 * count
    mx, m2, m3, m4, my, mxy, mxxy, myy = sx / n, sxx / n, sxxx / n, sxxxx / n, sy / n, sxy / n, sxxy / n, syy / n
    q = mx * mx
    u2 = m2 - q
    u3 = (m3 - (3.0 * mx) * m2) + (2.0 * mx) * q
    u4 = ((m4 - (4.0 * mx) * m3) + (6.0 * q) * m2) - (3.0 * q) * q
    cu = mxy - mx * my
    cv = ((mxxy - (2.0 * mx) * mxy) + q * my) - u2 * my
    k = u4 - u2 * u2
    det = u2 * k - u3 * u3
    tot = myy - my * my
    if my > 0 and tot > 0 and u2 >= MOD_MIN and det >= MOD_MIN * ((u2 * u2) * u2):
        b1, b2 = (cu * k - cv * u3) / det, (cv * u2 - cu * u3) / det
        res = tot - (b1 * cu + b2 * cv)
        ex, fit = 1.0 - res / tot, tot - res
        c1, c0 = b1 - (2.0 * b2) * mx, (my - b1 * mx) + b2 * (q - u2)
        depth = math.sqrt(fit if fit > 0.0 else 0.0) / my
        slope, curvature = (c1 / c0, b2 / c0) if c0 > 0 else (0.0, 0.0)
        if all(math.isfinite(v) for v in (ex, depth, slope, curvature)):
            out.update(explained=0.0 if ex < 0.0 else 1.0 if ex > 1.0 else ex, depth=depth, slope=slope, curvature=curvature)
    out["usn_db"] = _clamp_db(10.0 * math.log10(cdd / n)) if cdd > 0 else DB_MIN
    out["ripple_db"] = _clamp_db(10.0 * math.log10((cee / n) / (my * my))) if cee > 0 and my > 0 else DB_MIN
    if cee > 0 and cdd > 0:
        rho = ced / math.sqrt(cee * cdd)
        out["rho"] = 0.0 if not math.isfinite(rho) else -1.0 if rho < -1.0 else 1.0 if rho > 1.0 else rho
    out["multipath"] = out["explained"] >= cfg["explained_min"] and out["depth"] >= cfg["depth_min"]
    out["adjacent"] = abs(out["rho"]) >= cfg["rho_min"] and out["rho"] != 0.0
    out["side"] = (1 if out["rho"] > 0 else -1) if out["adjacent"] else 0
    return out


def reports(t: np.ndarray, cfg=None) -> dict:
    """what nrsc5hip_fm_impair returns after a session whose block records are t: {"windowed": {...}, "running": {...}, "blocks", "audio_blocks"}"""
    blocks = t.shape[0]
    audio = max(0, blocks - W)
    out = {"blocks": blocks, "audio_blocks": audio}
    for name, (s, count) in (("windowed", windowed(t, audio - 1) if audio > 0 else ([0.0] * NS, 0.0)), ("running", running(t, blocks))):
        out[name] = {**dict(zip(SUMS, (float(v) for v in s))), "count": count, **figures(s, count, cfg)}
    return out


def response_db(h: np.ndarray, f_hz) -> np.ndarray:
    """|H(f)| of taps at Fs1, in dB"""
    f = np.asarray(f_hz, dtype=np.float64)
    k = np.arange(h.size)
    H = np.exp(-2j * np.pi * np.outer(f / fm.FS1, k)) @ h.astype(np.float64)
    return 20 * np.log10(np.maximum(np.abs(H), 1e-30))
