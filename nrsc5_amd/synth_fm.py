"""Analog FM stereo host at 744 187.5 S/s from a programme of tones -- TEST SIGNAL SOURCE ONLY (nothing here is on the product path).

    MPX(t) = 0.9 [(L + R) / 2 + (L - R) / 2 * sin 2(wp t + th)] + pilot * sin(wp t + th)        (stereo; pilot 0.1 nominal)
    MPX(t) = 0.9 (L + R) / 2                                                                    (mono: pilot None)
    x(t)   = amp * exp(j 2 pi dev * integral of MPX)

L and R are sums of tones a cos(2 pi f t + ph).  Every term of the MPX is a sinusoid (a tone, a tone times the subcarrier as a sum and a
difference frequency, the pilot), so the phase integral is written in closed form and evaluated in float64 at every sample: no running
sum, no drift.  Pre-emphasis is applied as the tone's gain sqrt(1 + (2 pi f tau)^2); the pilot's frequency may be off by some ppm."""
from __future__ import annotations

import numpy as np

FS = 744187.5
PILOT_HZ = 19000.0
DEV_HZ = 75000.0


def _tones(tones, preemph_us):
    out = []
    for t in tones:
        f, a = float(t[0]), float(t[1])
        ph = float(t[2]) if len(t) > 2 else 0.0
        if preemph_us:
            a *= float(np.sqrt(1.0 + (2 * np.pi * f * preemph_us * 1e-6) ** 2))
        out.append((f, a, ph))
    return out


def mpx_terms(left, right, pilot=0.1, pilot_ppm=0.0, pilot_phase=0.0, preemph_us=None):
    """-> [(amplitude, frequency Hz, phase)] of the MPX as a sum of a * sin(2 pi f t + phase) terms"""
    L, R = _tones(left, preemph_us), _tones(right, preemph_us)
    terms = []
    for sign_d, tones in ((1.0, L), (-1.0, R)):
        for f, a, ph in tones:
            terms.append((0.9 * a / 2, f, ph + np.pi / 2))                     # cos = sin(. + pi/2): the sum path
            if pilot is not None:                                              # a cos(A) sin(B) = a/2 [sin(B + A) + sin(B - A)]
                fs2, th2 = 2 * PILOT_HZ * (1 + pilot_ppm * 1e-6), 2 * pilot_phase
                terms.append((sign_d * 0.9 * a / 4, fs2 + f, th2 + ph))
                terms.append((sign_d * 0.9 * a / 4, fs2 - f, th2 - ph))
    if pilot is not None:
        terms.append((float(pilot), PILOT_HZ * (1 + pilot_ppm * 1e-6), pilot_phase))
    return terms


def mpx(n: int, terms, fs: float = FS) -> np.ndarray:
    t = np.arange(n, dtype=np.float64) / fs
    out = np.zeros(n)
    for a, f, ph in terms:
        out += a * np.sin(2 * np.pi * f * t + ph)
    return out


def fm_phase(n: int, terms, fs: float = FS, dev_hz: float = DEV_HZ) -> np.ndarray:
    """2 pi dev * integral from 0 to t of the MPX, float64, closed form"""
    t = np.arange(n, dtype=np.float64) / fs
    out = np.zeros(n)
    for a, f, ph in terms:
        out += a * dev_hz / f * (np.cos(ph) - np.cos(2 * np.pi * f * t + ph))
    return out


def fm_host(n: int, left=(), right=(), pilot=0.1, pilot_ppm=0.0, pilot_phase=0.3, preemph_us=None, amp=8000.0, cnr_db=None, seed=0) -> np.ndarray:
    """int16 [n, 2]: the host as cs16 at 744 187.5 S/s.  cnr_db: white noise over the whole sampled band, carrier power / noise power"""
    terms = mpx_terms(left, right, pilot, pilot_ppm, pilot_phase, preemph_us)
    x = amp * np.exp(1j * fm_phase(n, terms))
    if cnr_db is not None:
        rng = np.random.default_rng(seed)
        s = amp * 10 ** (-cnr_db / 20) / np.sqrt(2)
        x = x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    return out


def fm_carrier(n: int, left=(), right=(), fs: float = FS, pilot=0.1, pilot_ppm=0.0, pilot_phase=0.3, preemph_us=None) -> np.ndarray:
    """complex128 [n]: the unit-amplitude host at any sample rate (for a wideband scene: scale, shift and add it)"""
    return np.exp(1j * fm_phase(n, mpx_terms(left, right, pilot, pilot_ppm, pilot_phase, preemph_us), fs))
