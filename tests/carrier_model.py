"""Float64 restatement of the carrier measurement's definition (include/nrsc5hip.h "carrier quality"), in numpy: what
nrsc5hip_fm_carrier* is checked against.  dtype=np.float32 runs the channel filter, the envelope and the discriminator in float32 (the block
sums stay double, as the definition has them): the reference's own estimate of how far a float32 implementation may sit from the float64 one.
The sums with a stated order (windowed, running) are restated in that order, so that they can be compared bit for bit."""
import numpy as np

from tests import fm_model as fm

BLOCK, W = fm.BLOCK, fm.W
DB_MIN, DB_MAX = -150.0, 150.0                 # NRSC5HIP_FM_CARRIER_DB_MIN / _MAX
FILTER_GAIN_DB = 5.34                          # -10 log10(sum hA^2): the in-filter CNR is this far above the CNR over the whole sampled band


def channel_filter(x: np.ndarray, ha: np.ndarray, dtype=np.float64):
    """z[m] = sum_i hA[i] x[2 m - i] -> (Re z, Im z) in dtype.  The taps are added one after the other, i ascending, as the definition writes the
    sum: in float32 that is what an implementation of the definition does (112 roundings in a row).  A library dot product with many partial
    accumulators, which np.convolve may use, is several times more accurate than any such implementation, and its error would not be an estimate
    of theirs: on a constant carrier every sample of a block carries the same rounding error, so a block sum shows it undiminished"""
    h = np.asarray(ha, dtype=np.float32).astype(dtype)
    m1 = (x.shape[0] + 1) // 2
    pad = np.zeros((h.size, 2), dtype)
    xp = np.concatenate([pad, x.astype(dtype), pad])            # xp[n + taps] = x[n]
    at = 2 * np.arange(m1, dtype=np.int64) + h.size
    zx, zy = np.zeros(m1, dtype), np.zeros(m1, dtype)
    for i in range(h.size):
        zx = zx + xp[at - i, 0] * h[i]
        zy = zy + xp[at - i, 1] * h[i]
    return zx, zy


def front(x: np.ndarray, ha: np.ndarray, dtype=np.float64):
    """x int16 [n, 2] -> r [ceil(n / 2)] (dtype), d [ceil(n / 2)] (dtype), block triples float64 [complete blocks][3]: s2, s4, s1"""
    m1 = (x.shape[0] + 1) // 2
    zx, zy = channel_filter(x, ha, dtype)
    r = (zx.astype(np.float64) ** 2 + (zy * zy).astype(np.float64)).astype(dtype)      # fma(zx, zx, zy zy)
    px, py = np.concatenate([np.zeros(1, dtype), zx[:-1]]), np.concatenate([np.zeros(1, dtype), zy[:-1]])
    re, im = (zx * px + zy * py).astype(dtype), (zy * px - zx * py).astype(dtype)        # z conj(z[m - 1])
    d = (np.arctan2(im, re).astype(dtype) * dtype(fm.DEV_SCALE)).astype(dtype)
    d[(re == 0) & (im == 0)] = 0
    d[0] = 0
    nb = m1 // BLOCK
    r64, d64 = r[:nb * BLOCK].astype(np.float64).reshape(nb, BLOCK), d[:nb * BLOCK].astype(np.float64).reshape(nb, BLOCK)
    t = np.stack([r64.sum(axis=1), (r64 * r64).sum(axis=1), d64.sum(axis=1)], axis=1) if nb else np.zeros((0, 3))
    return r, d, t


def block_sums_in_order(r: np.ndarray, d: np.ndarray) -> np.ndarray:
    """the block triples of given float32 r and d in the definition's order (lane l takes l + 64 i, i ascending, then the butterfly): bit for bit"""
    nb = r.size // BLOCK
    out = np.zeros((nb, 3))
    for j in range(nb):
        rr, dd = r[BLOCK * j:BLOCK * (j + 1)].astype(np.float64), d[BLOCK * j:BLOCK * (j + 1)].astype(np.float64)
        lanes = np.zeros((3, 64))
        for i in range((BLOCK + 63) // 64):
            seg = slice(64 * i, min(64 * i + 64, BLOCK))
            n = seg.stop - seg.start
            lanes[0, :n] += rr[seg]; lanes[1, :n] += rr[seg] * rr[seg]; lanes[2, :n] += dd[seg]
        out[j] = [butterfly(lanes[q]) for q in range(3)]
    return out


def butterfly(v: np.ndarray) -> float:
    """64 lanes: v += v[lane ^ s] for s = 32, 16, .. 1; every lane ends with the same bits"""
    v = np.asarray(v, dtype=np.float64).copy()
    idx = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ s]
    assert np.all(v == v[0]) or np.any(np.isnan(v))
    return float(v[0])


def window32() -> np.ndarray:
    """the pilot's window as the device reads it: float32 values, in double"""
    return fm.pilot_window().astype(np.float32).astype(np.float64)


def windowed(t: np.ndarray, ja: int):
    """the windowed triple of audio block ja from the block triples t [blocks][3] (blocks > ja + W) -> (sum2, sum4, sum1, count)"""
    win = window32()
    out = []
    for q in range(3):
        lanes = np.zeros(64)
        for lane in range(2 * W + 1):
            jb = ja + lane - W
            if jb >= 0:
                lanes[lane] = t[jb, q] * win[lane]
        out.append(butterfly(lanes))
    count = 0.0
    for w in win:
        count += float(w)
    return out[0], out[1], out[2], count


def running(t: np.ndarray, blocks: int):
    """blocks [0, blocks) added one after the other -> (sum2, sum4, sum1, count)"""
    s = [0.0, 0.0, 0.0]
    for j in range(blocks):
        for q in range(3):
            s[q] = s[q] + float(t[j, q])
    return s[0], s[1], s[2], float(blocks)


def figures(sum2: float, sum4: float, sum1: float, count: float) -> dict:
    """level_db, cnr_db, offset_hz of a triple: the binding's formula"""
    if not count > 0:
        return {"level_db": 0.0, "cnr_db": 0.0, "offset_hz": 0.0}
    P, K = sum2 / (540.0 * count), sum4 / (540.0 * count)
    q = 2.0 * P * P - K
    S = np.sqrt(q) if q > 0 else 0.0
    N = P - S
    level = cnr = DB_MIN
    if S > 0 and P > 0:
        level = 10.0 * np.log10(S / 32768.0 ** 2)
        cnr = 10.0 * np.log10(S / N) if N > 0 else DB_MAX
    return {"level_db": float(min(max(level, DB_MIN), DB_MAX)), "cnr_db": float(min(max(cnr, DB_MIN), DB_MAX)),
            "offset_hz": float(75000.0 * sum1 / (540.0 * count))}


def reports(t: np.ndarray) -> dict:
    """what nrsc5hip_fm_carrier returns after a session whose block triples are t: {"windowed": {...}, "running": {...}, "blocks", "audio_blocks"}"""
    blocks = t.shape[0]
    audio = max(0, blocks - W)
    out = {"blocks": blocks, "audio_blocks": audio}
    for name, tr in (("windowed", windowed(t, audio - 1) if audio > 0 else (0.0, 0.0, 0.0, 0.0)), ("running", running(t, blocks))):
        out[name] = {"sum2": tr[0], "sum4": tr[1], "sum1": tr[2], "count": tr[3], **figures(*tr)}
    return out
