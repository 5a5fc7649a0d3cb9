"""Analog FM stereo host at 744 187.5 S/s from a programme of tones -- TEST SIGNAL SOURCE ONLY (nothing here is on the product path).

    MPX(t) = 0.9 [(L + R) / 2 + (L - R) / 2 * sin 2(wp t + th)] + pilot * sin(wp t + th)        (stereo; pilot 0.1 nominal)
    MPX(t) = 0.9 (L + R) / 2                                                                    (mono: pilot None)
    x(t)   = amp * exp(j 2 pi dev * integral of MPX)

L and R are sums of tones a cos(2 pi f t + ph).  Every term of the MPX is a sinusoid (a tone, a tone times the subcarrier as a sum and a
difference frequency, the pilot), so the phase integral is written in closed form and evaluated in float64 at every sample: no running
sum, no drift.  Pre-emphasis is applied as the tone's gain sqrt(1 + (2 pi f tau)^2); the pilot's frequency may be off by some ppm.

RDS / RBDS (the keyword `rds`): a 57 kHz subcarrier, 3 x the pilot's phase (its ppm included) plus `phase`, carrying the biphase symbols of a
repeating list of groups -- check words with the offset words, differential encoding, two impulses per bit shaped with the closed-form h(t) of
the standard (RdsSignal).  That term alone is no sinusoid: its phase integral is a float64 Simpson sum (RdsSignal.phase_integral).

EAS alerts (the keyword `same`): SAME bursts as mono AFSK on the sum path (SameSignal) -- 16 bytes 0xAB and the text, least significant bit
first, mark 6250/3 Hz and space 1562.5 Hz at 3125/6 bit/s.  Every bit holds a whole number of tone cycles, so the tone restarts at each bit
boundary without a step and its phase integral is closed form: whole bits contribute nothing."""
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


class Terms(list):
    """the MPX's sinusoids, with the RDS term and the SAME bursts beside them"""
    rds = None
    same = None


RDS_POLY = 0x5B9                                   # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
RDS_OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
RDS_SPAN = 12                                      # bit periods of h(t) kept on either side of an impulse


def rds_checkword(data: int) -> int:
    """the 10 check bits of a 16-bit information word: remainder of data * x^10 by the generator, before the offset word"""
    reg = (data & 0xFFFF) << 10
    for k in range(25, 9, -1):
        if reg >> k & 1:
            reg ^= RDS_POLY << (k - 10)
    return reg & 0x3FF


def rds_bits(groups) -> np.ndarray:
    """uint8 [104 * len(groups)]: the groups (a, b, c, d) as transmitted, most significant bit first, block 3 with C' when b names version B"""
    out = []
    for a, b, c, d in groups:
        for word, off in ((a, "A"), (b, "B"), (c, "C'" if b >> 11 & 1 else "C"), (d, "D")):
            v = (word & 0xFFFF) << 10 | (rds_checkword(word) ^ RDS_OFFSETS[off])
            out.extend(v >> k & 1 for k in range(25, -1, -1))
    return np.array(out, dtype=np.uint8)


def rds_h(u: np.ndarray) -> np.ndarray:
    """h at u = 4 t / T: sinc(u + 1/2) + sinc(u - 1/2) = cos(pi u) / (pi (1/4 - u^2)), the cosine-shaped spectrum on |f| <= 2 / T"""
    return np.sinc(u + 0.5) + np.sinc(u - 0.5)


def _rds_norm() -> float:
    u = np.linspace(-4.0, 6.0, 20001)
    return float(np.max(np.abs(rds_h(u) - rds_h(u - 2.0))))


class RdsSignal:
    """m(t) sin(3 (wp t + th) + phase): m(t) = sum_i (2 e_i - 1) g(t - (i + bit_offset) T) / max|g|, g(t) = h(t) - h(t - T / 2), e the
    differentially encoded bits of the repeating group list.  T is 16 pilot cycles, or 1 / (1187.5 (1 + clock_ppm 1e-6)) s when clock_ppm is
    given.  dev_hz is the peak deviation of an isolated symbol.  h is cut RDS_SPAN bit periods from its impulse (|h| < 1.4e-4 there)."""

    def __init__(self, groups, pilot_hz, pilot_phase, dev_hz=2000.0, phase=0.0, clock_ppm=None, bit_offset=0.0):
        self.groups = [tuple(int(w) & 0xFFFF for w in g) for g in groups]
        self.dev_hz, self.phase, self.bit_offset = float(dev_hz), float(phase), float(bit_offset)
        self.pilot_hz, self.pilot_phase = float(pilot_hz), float(pilot_phase)
        self.bit_hz = self.pilot_hz / 16 if clock_ppm is None else PILOT_HZ / 16 * (1 + clock_ppm * 1e-6)
        self.norm = _rds_norm()
        self._frame = rds_bits(self.groups)

    def bits(self, n: int) -> np.ndarray:
        """the first n data bits (the group list repeats)"""
        return np.resize(self._frame, n)

    def envelope(self, t: np.ndarray) -> np.ndarray:
        """m(t): cos(pi u) is common to every impulse (they sit 2 apart in u), so one cosine and 4 RDS_SPAN + 1 divisions per sample"""
        t = np.asarray(t, dtype=np.float64)
        u = 4.0 * (t * self.bit_hz - self.bit_offset)                       # impulse j (two per bit) at u = 2 j
        nbits = int(np.ceil(max(float(u.max()), 0.0) / 4)) + RDS_SPAN + 2 if u.size else 1
        e = np.bitwise_xor.accumulate(self.bits(nbits)).astype(np.float64) * 2 - 1
        pad = 2 * RDS_SPAN + 2
        c = np.zeros(2 * nbits + 2 * pad)
        c[pad:pad + 2 * nbits:2] = e
        c[pad + 1:pad + 2 * nbits:2] = -e
        out = np.empty(t.size)
        k = np.arange(-2 * RDS_SPAN, 2 * RDS_SPAN + 1)
        for a in range(0, t.size, 1 << 16):
            uu = u[a:a + (1 << 16)]
            j0 = np.floor(uu / 2 + 0.5).astype(np.int64)
            du = (uu - 2 * j0)[:, None] - 2 * k[None, :]                   # u relative to impulse j0 + k
            den = np.pi * (0.25 - du * du)
            near = np.abs(den) < 1e-6
            w = np.cos(np.pi * uu)[:, None] / np.where(near, 1.0, den)
            if near.any():
                w[near] = rds_h(du[near])
            idx = j0[:, None] + k[None, :] + pad
            ok = (idx >= 0) & (idx < c.size)
            out[a:a + uu.size] = np.sum(np.where(ok, c[np.clip(idx, 0, c.size - 1)], 0.0) * w, axis=1)
        return out / self.norm

    def value(self, t: np.ndarray) -> np.ndarray:
        t = np.asarray(t, dtype=np.float64)
        return self.envelope(t) * np.sin(3 * (2 * np.pi * self.pilot_hz * t + self.pilot_phase) + self.phase)

    def phase_integral(self, n: int, fs: float, over: int = 8) -> np.ndarray:
        """integral of value() from 0 to k / fs, k < n: composite Simpson with `over` (even, >= 8) steps per sample, float64.  Error: per second of
        signal at most hs^4 / 180 * max|value''''| <= (2 pi 59.4 kHz hs)^4 / 180 * 1.6 with hs = 1 / (over fs) -- 1.4e-7 s/s at 744 187.5 S/s, so
        the carrier's phase 2 pi dev_hz * integral is off by less than 1.8e-3 rad per second at dev_hz = 2 kHz if every step erred alike; the
        integrand alternates and the measured error (against over = 32) is below 1e-6 rad.  The running sum of n float64 terms adds ~1e-13."""
        assert over >= 8 and over % 2 == 0
        if n <= 1:
            return np.zeros(n)
        t = np.arange((n - 1) * over + 1, dtype=np.float64) / (fs * over)
        v = self.value(t)
        w = np.full(over + 1, 2.0)
        w[1::2] = 4.0
        w[0] = w[-1] = 1.0
        cells = v[:-1].reshape(n - 1, over)
        per = cells @ w[:-1] + v[over::over] * w[-1]
        out = np.zeros(n)
        np.cumsum(per / (3.0 * fs * over), out=out[1:])
        return out


SAME_BIT_HZ = 3125.0 / 6.0
SAME_PREAMBLE = bytes([0xAB] * 16)


def same_bits(text, preamble: bytes = SAME_PREAMBLE) -> np.ndarray:
    """uint8 [8 * (16 + len(text))]: a SAME burst as transmitted, the preamble and then the text, every byte least significant bit first"""
    raw = preamble + (text.encode("latin-1") if isinstance(text, str) else bytes(text))
    return np.unpackbits(np.frombuffer(raw, dtype=np.uint8), bitorder="little")


class SameSignal:
    """level * sin(2 pi f_b (t - t_b)) inside bit b of a burst (f_b = 4 / T for a 1, 3 / T for a 0, t_b the bit's start), 0 between the bursts.
    bursts: [(start_s, text), ...], not overlapping; T = 6 / 3125 s / (1 + clock_ppm 1e-6) -- the tones move with the bit clock, as they do in
    an encoder that derives both from one oscillator.  preemph_us: each tone at its pre-emphasised level"""

    def __init__(self, bursts, level=0.3, clock_ppm=0.0, preemph_us=None):
        self.level, self.bit_hz = float(level), SAME_BIT_HZ * (1 + float(clock_ppm) * 1e-6)
        self.bursts = [(float(t0), same_bits(text)) for t0, text in bursts]
        g = lambda f: float(np.sqrt(1.0 + (2 * np.pi * f * preemph_us * 1e-6) ** 2)) if preemph_us else 1.0
        self.gain = (g(3 * self.bit_hz), g(4 * self.bit_hz))            # space, mark
        ends = [t0 + b.size / self.bit_hz for t0, b in self.bursts]
        assert all(a <= t0 for a, (t0, _) in zip(ends, self.bursts[1:])), "bursts overlap"

    def _tone(self, t: np.ndarray):
        """-> (amplitude, frequency, time since the bit's start) of every t; amplitude 0 outside the bursts"""
        t = np.asarray(t, dtype=np.float64)
        amp, f, tau = np.zeros(t.shape), np.ones(t.shape), np.zeros(t.shape)
        for t0, bits in self.bursts:
            u = (t - t0) * self.bit_hz
            k = np.floor(u).astype(np.int64)
            on = (u >= 0) & (k < bits.size)
            b = bits[np.clip(k, 0, bits.size - 1)]
            amp = np.where(on, self.level * np.where(b == 1, self.gain[1], self.gain[0]), amp)
            f = np.where(on, np.where(b == 1, 4.0, 3.0) * self.bit_hz, f)
            tau = np.where(on, (u - k) / self.bit_hz, tau)
        return amp, f, tau

    def value(self, t: np.ndarray) -> np.ndarray:
        amp, f, tau = self._tone(t)
        return amp * np.sin(2 * np.pi * f * tau)

    def phase_integral(self, t: np.ndarray) -> np.ndarray:
        """integral of value() from 0 to t: the part of the bit t lies in, every whole bit integrating to zero"""
        amp, f, tau = self._tone(t)
        return amp / (2 * np.pi * f) * (1.0 - np.cos(2 * np.pi * f * tau))


def rds_groups(pi: int, ps: str = "        ", text: str | None = None, clock=None, pty: int = 0, tp: int = 0, ta: int = 0, ms: int = 1, ab: int = 0,
               version_b: bool = False, extra=()) -> list:
    """a group schedule [(a, b, c, d), ...]: the four 0A (or 0B) groups of the name, then the text as 2A (2B) groups (ended by 0x0D when shorter
    than the 64 (32) characters), then one 4A group for clock = (mjd, hour, minute, offset in half hours), then `extra` as they are"""
    ver = 1 if version_b else 0
    head = lambda gt, v: (gt & 15) << 12 | v << 11 | (tp & 1) << 10 | (pty & 31) << 5
    name = ps.encode("latin-1").ljust(8)[:8]
    out = []
    for seg in range(4):
        b = head(0, ver) | (ta & 1) << 4 | (ms & 1) << 3 | (1 if seg == 3 else 0) << 2 | seg
        out.append((pi, b, pi if ver else 0xE0CD, name[2 * seg] << 8 | name[2 * seg + 1]))
    if text is not None:
        per = 2 if ver else 4
        raw = text.encode("latin-1")[:16 * per]
        if len(raw) < 16 * per:
            raw += b"\r"
        raw = raw.ljust(-(-len(raw) // per) * per)
        for seg in range(len(raw) // per):
            b = head(2, ver) | (ab & 1) << 4 | seg
            q = raw[per * seg:per * seg + per]
            out.append((pi, b, pi, q[0] << 8 | q[1]) if ver else (pi, b, q[0] << 8 | q[1], q[2] << 8 | q[3]))
    if clock is not None:
        mjd, hour, minute, off = clock
        b = head(4, 0) | (mjd >> 15 & 3)
        out.append((pi, b, (mjd & 0x7FFF) << 1 | (hour >> 4 & 1), (hour & 15) << 12 | (minute & 63) << 6 | (1 if off < 0 else 0) << 5 | (abs(off) & 31)))
    out.extend(tuple(g) for g in extra)
    return out


def mpx_terms(left, right, pilot=0.1, pilot_ppm=0.0, pilot_phase=0.0, preemph_us=None, rds=None, same=None):
    """-> [(amplitude, frequency Hz, phase)] of the MPX as a sum of a * sin(2 pi f t + phase) terms; with `rds` the list also carries the
    RDS term as its attribute .rds (an RdsSignal), with `same` = dict(bursts=[(start_s, text), ...], level=..) the SAME bursts as .same (a
    SameSignal), which mpx() and fm_phase() add"""
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
    if rds is not None:
        terms = Terms(terms)
        terms.rds = RdsSignal(pilot_hz=PILOT_HZ * (1 + pilot_ppm * 1e-6), pilot_phase=pilot_phase, **rds)
    if same is not None:
        terms = terms if isinstance(terms, Terms) else Terms(terms)
        terms.same = SameSignal(preemph_us=preemph_us, **same)
    return terms


def mpx(n: int, terms, fs: float = FS) -> np.ndarray:
    t = np.arange(n, dtype=np.float64) / fs
    out = np.zeros(n)
    for a, f, ph in terms:
        out += a * np.sin(2 * np.pi * f * t + ph)
    rds = getattr(terms, "rds", None)
    if rds is not None:
        out += rds.dev_hz / DEV_HZ * rds.value(t)
    same = getattr(terms, "same", None)
    if same is not None:
        out += same.value(t)
    return out


def fm_phase(n: int, terms, fs: float = FS, dev_hz: float = DEV_HZ, delay_s: float = 0.0) -> np.ndarray:
    """2 pi dev * integral from 0 to t of the MPX, float64, closed form; delay_s: evaluated at t - delay_s (a delayed ray of a host of tones)"""
    t = np.arange(n, dtype=np.float64) / fs
    if delay_s:
        if getattr(terms, "rds", None) is not None or getattr(terms, "same", None) is not None:
            raise ValueError("a delayed ray is available for hosts of tones only: not with rds or same")
        t = t - delay_s
    out = np.zeros(n)
    for a, f, ph in terms:
        out += a * dev_hz / f * (np.cos(ph) - np.cos(2 * np.pi * f * t + ph))
    rds = getattr(terms, "rds", None)
    if rds is not None:
        out += 2 * np.pi * dev_hz * (rds.dev_hz / DEV_HZ) * rds.phase_integral(n, fs)
    same = getattr(terms, "same", None)
    if same is not None:
        out += 2 * np.pi * dev_hz * same.phase_integral(t)
    return out


def _with_rays(n: int, terms, fs: float, rays) -> np.ndarray:
    """the unit-amplitude carrier plus a * exp(j (phase(t - tau) + phi)) per ray (a, tau_s, phi): the phase integral in closed form at the shifted
    time; the rotation of the carrier itself over tau is part of phi"""
    x = np.exp(1j * fm_phase(n, terms, fs))
    for a, tau, phi in rays or ():
        x = x + float(a) * np.exp(1j * (fm_phase(n, terms, fs, delay_s=float(tau)) + float(phi)))
    return x


def fm_host(n: int, left=(), right=(), pilot=0.1, pilot_ppm=0.0, pilot_phase=0.3, preemph_us=None, amp=8000.0, cnr_db=None, seed=0, rds=None, same=None,
            rays=None) -> np.ndarray:
    """int16 [n, 2]: the host as cs16 at 744 187.5 S/s.  cnr_db: white noise over the whole sampled band, power of the direct carrier / noise power.
    rays: [(a, tau_s, phi), ...], delayed copies of relative amplitude a (multipath); hosts of tones only, refused together with rds / same"""
    if rays and (rds is not None or same is not None):
        raise ValueError("rays: hosts of tones only, not together with rds or same")
    terms = mpx_terms(left, right, pilot, pilot_ppm, pilot_phase, preemph_us, rds, same)
    x = amp * _with_rays(n, terms, FS, rays)
    if cnr_db is not None:
        rng = np.random.default_rng(seed)
        s = amp * 10 ** (-cnr_db / 20) / np.sqrt(2)
        x = x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    return out


def fm_carrier(n: int, left=(), right=(), fs: float = FS, pilot=0.1, pilot_ppm=0.0, pilot_phase=0.3, preemph_us=None, rds=None, same=None, rays=None) -> np.ndarray:
    """complex128 [n]: the unit-amplitude host at any sample rate (for a wideband scene: scale, shift and add it); rays as in fm_host (the direct
    carrier keeps amplitude 1)"""
    if rays and (rds is not None or same is not None):
        raise ValueError("rays: hosts of tones only, not together with rds or same")
    return _with_rays(n, mpx_terms(left, right, pilot, pilot_ppm, pilot_phase, preemph_us, rds, same), fs, rays)
