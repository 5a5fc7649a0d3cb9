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
