"""float64 restatement of the wideband channelizer's definition (include/nrsc5hip.h, nrsc5hip_chan_*) for the tests: the same
integer phase and index arithmetic as the library, its own float32 prototype table (read back with nrsc5hip_chan_taps), and every
sum in float64 -- plus the ideal channelizer (the exact Kaiser prototype at the exact fractional time, no table)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

OUT_RATE = Fraction(1488375, 2)
PASS_HZ, STOP_HZ, DESIGN_ATTEN_DB = 198.5e3, 545.8e3, 80.0


def ratio(rate_num: int, rate_den: int):
    r = Fraction(rate_num, rate_den) / OUT_RATE
    return r.numerator, r.denominator


SPAN_MAX = 4096
CLIP_GAIN = 20.0        # on an output of about 1500 LSB rms (level()): each component has sigma 21 000, about a fifth of the outputs clip

# The rates at which the kernel's configuration changes (tile(): mt 256 / 64 / 32, the block of 64 work-items over a tile of 32), the
# resampling ratio is 1, the phase count is clamped to 4096, the rate is a fraction, and the taps run into the hundreds.
RATE_EDGE_CASES = [Fraction(1488375, 2), Fraction(1000000), Fraction(20000000, 3), Fraction(30720000), Fraction(40000000),
                   Fraction(56000000), Fraction(64000000)]


def rate_id(rate) -> str:
    r = Fraction(rate)
    return str(r.numerator) if r.denominator == 1 else f"{r.numerator}over{r.denominator}"


def tile(P: int, Q: int, T: int):
    """the tile rule of nrsc5hip_chan_create -> (outputs per tile mt, input samples one tile may span)"""
    mt = 256
    while mt > 16 and (mt - 1) * P // Q + T + 2 > SPAN_MAX:
        mt //= 2
    return mt, (mt - 1) * P // Q + T + 2


def case_size(rate, T: int, k: int = 1):
    """-> (n, chunks): n input samples whose outputs span at least 3.5 tiles after T samples of start-up -- and number at least 2000 / k
    per channel, so that 1 % of the k channels' values is 40 values and not 2 --, pushed as three chunks: the first ends inside a tile
    (not on a tile boundary), the second is shorter than T"""
    r = Fraction(rate)
    P, Q = ratio(r.numerator, r.denominator)
    mt, _ = tile(P, Q, T)
    M = max(-(-7 * mt // 2), -(-2000 // k))
    n = -(-M * P // Q) + T + T // 2
    assert outputs_total(n, P, Q, T) >= M
    first = n // 3
    while outputs_total(first, P, Q, T) % mt == 0:
        first += 1
    assert 5 < T and 0 < first < n - 5
    return n, [first, 5, n - first - 5]


def level(rate, target_rms: float = 1500.0) -> float:
    """sigma per component (library scale) of white Gaussian input for which one channel's output has about target_rms: the output
    power of white noise is 2 sigma^2 sum(h^2), and sum(h^2) of one phase is close to the prototype's two-sided width 2 fc =
    (PASS_HZ + STOP_HZ) / fs of the band (measured 0.91 of it at 64 MS/s; the whole band at 744 187.5 S/s)"""
    return target_rms / np.sqrt(2.0 * min(1.0, (PASS_HZ + STOP_HZ) / float(Fraction(rate))))


def raw_noise(fmt: int, n: int, seed: int, sigma: float) -> np.ndarray:
    """interleaved raw white samples of rms `sigma` per component in the library's scale: Gaussian (cs16 saturates at +-3.3 sigma for
    the largest level()).  cu8 holds at most 127 * 64 per component, and a Gaussian of more than a third of that would lose its power
    to saturation (at 64 MS/s the output rms would fall to 800 LSB): such levels are drawn as 127 +- a with a random sign and a
    magnitude spread over some 20 byte values below a = min(127, sigma / 64), still white, about 1100 LSB rms out at 64 MS/s."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(2 * n)
    if fmt == 0 and sigma / 64.0 > 40.0:
        mag = np.clip(min(127.0, sigma / 64.0) - np.abs(8.0 * rng.standard_normal(2 * n)), 0, 127)
        return np.rint(127 + np.sign(g) * mag).astype(np.uint8)
    if fmt == 0:
        return np.clip(np.rint(127 + sigma / 64.0 * g), 0, 255).astype(np.uint8)
    if fmt == 1:
        return np.clip(np.rint(sigma * g), -32768, 32767).astype(np.int16)
    return (sigma / 32768.0 * g).astype(np.float32)


def edge_case_params(formats=(0, 1, 2)):
    """(rate, fmt, K) of the model comparison over the rate range: every format at the two end rates, cs16 at the others; K odd, with
    a one-channel tail of the two-channel FIR loop (1, 3, 9, 11) and a partial last group of eight (9, 11)"""
    out = []
    for rate in RATE_EDGE_CASES:
        for fmt in (formats if rate in (RATE_EDGE_CASES[0], RATE_EDGE_CASES[-1]) else (1,)):
            for k in (1, 3, 9, 11):
                out.append((rate, fmt, k))
    return out


def edge_case_id(p) -> str:
    return f"{rate_id(p[0])}-{('cu8', 'cs16', 'cf32')[p[1]]}-K{p[2]}"


def assert_equals_model(got: np.ndarray, got_clips, want: np.ndarray, clips, y=None, rms_range=None):
    """the rule a channelizer's output is held to against model(): same shape, largest difference 1 LSB, at most 1 % of the values
    differing, equal clip counts; rms_range: the model's output rms of every channel (after the first quarter) lies inside it.
    -> (largest difference, share of values differing, rms per channel)"""
    assert got.shape == want.shape, (got.shape, want.shape)
    rms = None
    if y is not None:
        rms = np.sqrt(np.mean(np.abs(y[:, y.shape[1] // 4:]) ** 2, axis=1))
        if rms_range is not None:
            assert np.all(rms > rms_range[0]) and np.all(rms < rms_range[1]), rms
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    worst, share = int(diff.max()), float(np.mean(diff != 0))
    print(f"largest difference {worst} LSB, share of values differing {100 * share:.4f} %, clips {np.asarray(clips).tolist()}")
    assert worst <= 1, worst
    assert share <= 0.01, share
    assert np.array_equal(np.asarray(got_clips), np.asarray(clips)), (got_clips, clips)
    return worst, share, rms


def scaled(raw: np.ndarray, fmt: int) -> np.ndarray:
    """interleaved raw samples -> complex128 in the library's scale (cu8: (b - 127) * 64, cs16: as is, cf32: v * 32768)"""
    v = raw.astype(np.float64)
    if fmt == 0:
        v = (v - 127.0) * 64.0
    elif fmt == 2:
        v = v * 32768.0
    return v[0::2] + 1j * v[1::2]


def steps(offsets_hz, rate_num: int, rate_den: int) -> np.ndarray:
    fs = rate_num / rate_den
    return np.array([int(np.floor(f / fs * 2.0 ** 32 + 0.5)) for f in offsets_hz], dtype=np.int64)


def outputs_total(n: int, P: int, Q: int, T: int) -> int:
    a1 = n - T // 2
    return 0 if a1 <= 0 else (a1 * Q + P - 1) // P


def positions(M: int, P: int, Q: int, L: int):
    """(anchor i, phase row p) of outputs 0..M-1, as the kernel computes them"""
    q = np.arange(M, dtype=object) * P
    i = np.array([int(v // Q) for v in q], dtype=np.int64)
    r = np.array([int(v % Q) for v in q], dtype=np.int64)
    p = (r * L + Q // 2) // Q
    up = p == L
    i[up] += 1
    p[up] = 0
    return i, p, r


def mixed(x: np.ndarray, s: int) -> np.ndarray:
    n = np.arange(x.size, dtype=np.int64)
    th = (n * (s % (1 << 32))) % (1 << 32)
    th = np.where(th >= 1 << 31, th - (1 << 32), th).astype(np.float64)
    return x * np.exp(-2j * np.pi * th / 2.0 ** 32)


def _fir(v: np.ndarray, i: np.ndarray, coef: np.ndarray, T: int) -> np.ndarray:
    """sum_j v[i - T/2 + 1 + j] * coef[m, j], samples outside [0, len(v)) zero"""
    pad = np.concatenate([np.zeros(T, dtype=v.dtype), v, np.zeros(T + 2, dtype=v.dtype)])
    idx = (i - T // 2 + 1 + T)[:, None] + np.arange(T)[None, :]
    return np.sum(pad[idx] * coef, axis=1)


def model(x: np.ndarray, rate_num: int, rate_den: int, offsets_hz, gains, table: np.ndarray):
    """-> (int16 [K, M, 2] as the definition rounds and clamps, float64 [K, M] complex before rounding, clip counts [K])"""
    L, T = table.shape
    P, Q = ratio(rate_num, rate_den)
    M = outputs_total(x.size, P, Q, T)
    i, p, _ = positions(M, P, Q, L)
    coef = table.astype(np.float64)[p]
    gains = np.ones(len(offsets_hz)) if gains is None else np.asarray(gains, dtype=np.float64)
    ys, outs, clips = [], [], []
    for k, s in enumerate(steps(offsets_hz, rate_num, rate_den)):
        y = gains[k] * _fir(mixed(x, int(s)), i, coef, T)
        r = np.stack([np.rint(y.real), np.rint(y.imag)], axis=-1)
        clips.append(int(np.sum(np.any((r > 32767) | (r < -32768), axis=-1))))
        outs.append(np.clip(r, -32768, 32767).astype(np.int16))
        ys.append(y)
    return np.stack(outs), np.stack(ys), np.array(clips)


def kaiser_h(tau: np.ndarray, fs: float, T: int) -> np.ndarray:
    """the exact prototype: Kaiser-windowed sinc, cut-off half-way through the transition band, support (-T/2, T/2)"""
    beta = 0.1102 * (DESIGN_ATTEN_DB - 8.7)
    fc = 0.5 * (PASS_HZ + STOP_HZ) / fs
    u = 2.0 * tau / T
    w = np.where(np.abs(u) < 1, np.i0(beta * np.sqrt(np.clip(1 - u * u, 0, None))) / np.i0(beta), 0.0)
    return 2 * fc * np.sinc(2 * fc * tau) * w


def ideal(x: np.ndarray, rate_num: int, rate_den: int, offsets_hz, gains, T: int, M: int) -> np.ndarray:
    """float64 channelizer with the exact h at the exact time t_m (no table, no phase quantisation, no rounding): complex [K, M]"""
    P, Q = ratio(rate_num, rate_den)
    fs = rate_num / rate_den
    q = np.arange(M, dtype=object) * P
    i = np.array([int(v // Q) for v in q], dtype=np.int64)
    frac = np.array([float(Fraction(int(v % Q), Q)) for v in q])
    coef = kaiser_h(frac[:, None] + T // 2 - 1 - np.arange(T)[None, :], fs, T)
    gains = np.ones(len(offsets_hz)) if gains is None else np.asarray(gains, dtype=np.float64)
    off = np.asarray(offsets_hz, dtype=np.float64)
    n = np.arange(x.size)
    return np.stack([gains[k] * _fir(x * np.exp(-2j * np.pi * off[k] * n / fs), i, coef, T) for k in range(len(off))])
