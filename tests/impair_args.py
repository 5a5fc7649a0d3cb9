"""Seeded inputs of the reception-impairment tests (tests/impair_checks.py): cs16 hosts at 744 187.5 S/s, each asserted to hold what it is named
for, with the float64 model's output (tests/impair_model.py) computed once per input and shared; analyse() asserts, on that model, what each
input is named for -- the definition is judged on the CPU before any library is.  A session is fm_args.N = 120 000 input samples: 111 blocks,
95 audio blocks.  Every scene stays inside int16 but "fullscale", which is there to clip: clipping is an impairment of its own."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import carrier_model as cm, fm_args as fa, impair_model as im

N = fa.N
AMP = 6000.0                                                       # with a neighbour 10 dB above: 6000 + 18 974 < 32 767
PROG = dict(left=[(1000.0, 0.5)], right=[(3000.0, 0.4)], pilot=0.1)
# The neighbour is an ordinary station: modulated close to full deviation.  Its carrier, 200 kHz away, lies in the channel filter's stopband; what
# reaches the detector is the part of its spectrum that its own modulation swings below 129 kHz, so rho at a given level grows with the neighbour's
# deviation (a silent neighbour is invisible, one modulated like PROG reads |rho| 0.43 .. 0.50 at -10 dB, this one 0.80)
NEIGHBOUR = dict(left=[(700.0, 0.7)], right=[(2200.0, 0.6)], pilot=0.1, pilot_phase=1.1)
RAY5 = (0.3, 5e-6, 2.0)


def _case(prog=PROG, amp=AMP, cnr=None, rays=(), adj=None, seed=0):
    """cnr: in-filter CNR in dB (5.34 dB above the CNR over the whole sampled band); adj: (offset Hz, level dB against the carrier)"""
    return dict(prog=prog, amp=amp, cnr=cnr, rays=tuple(rays), adj=adj, seed=seed)


CASES = {
    "clean": _case(),
    "noise40": _case(cnr=40.0, seed=40), "noise30": _case(cnr=30.0, seed=30), "noise20": _case(cnr=20.0, seed=20), "noise10": _case(cnr=10.0, seed=10),
    "ray2us": _case(rays=[(0.3, 2e-6, 1.0)]), "ray5us": _case(rays=[RAY5]), "ray10us": _case(rays=[(0.5, 10e-6, 0.0)]),
    "ray3us_weak": _case(rays=[(0.1, 3e-6, 0.5)]), "ray5us_noise30": _case(rays=[(0.5, 5e-6, 2.0)], cnr=30.0, seed=31),
    "adj+200_-10": _case(adj=(200e3, -10.0)), "adj+200_0": _case(adj=(200e3, 0.0)), "adj+200_+10": _case(adj=(200e3, 10.0)),
    "adj-200_-10": _case(adj=(-200e3, -10.0)), "adj-200_0": _case(adj=(-200e3, 0.0)), "adj-200_+10": _case(adj=(-200e3, 10.0)),
    "adj+200_+10_noise20": _case(adj=(200e3, 10.0), cnr=20.0, seed=21),
    "adj+200_+10_ray5us": _case(adj=(200e3, 10.0), rays=[RAY5]),
    "unmodulated": _case(prog=dict(pilot=None)),
    "zero": _case(prog=None, amp=0.0),
    "fullscale": _case(amp=40000.0),
}
RAY_CASES = [k for k, v in CASES.items() if v["rays"]]
ADJ_CASES = [k for k, v in CASES.items() if v["adj"]]
ADJ_QUIET = [k for k in ADJ_CASES if CASES[k]["cnr"] is None]               # a neighbour without added noise
PLAIN_CASES = [k for k, v in CASES.items() if not v["rays"] and not v["adj"]]
MULTI = {1: ["ray5us"], 3: ["clean", "adj-200_0", "ray10us"],
         9: ["noise20", "ray2us", "adj+200_+10", "zero", "fullscale", "unmodulated", "adj+200_+10_ray5us", "clean", "ray5us"]}


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """int16 [N, 2], read-only"""
    c = CASES[name]
    if c["prog"] is None:
        x = np.zeros(N, dtype=np.complex128)
    else:
        p = c["prog"]
        terms = sf.mpx_terms(p.get("left", ()), p.get("right", ()), p.get("pilot", 0.1), 0.0, p.get("pilot_phase", 0.3))
        x = c["amp"] * sf._with_rays(N, terms, sf.FS, c["rays"])
        if c["adj"]:
            off, db = c["adj"]
            x = x + c["amp"] * 10 ** (db / 20) * sf.fm_carrier(N, **NEIGHBOUR) * np.exp(2j * np.pi * off * np.arange(N) / sf.FS)
        if c["cnr"] is not None:
            rng = np.random.default_rng(c["seed"])
            s = c["amp"] * 10 ** (-(c["cnr"] - cm.FILTER_GAIN_DB) / 20) / np.sqrt(2)
            noise = s * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
            got = 10 * np.log10(c["amp"] ** 2 / np.mean(np.abs(noise) ** 2)) + cm.FILTER_GAIN_DB     # this realisation's power, as an in-filter CNR
            assert abs(got - c["cnr"]) < 0.1, (name, got)
            x = x + noise
    out = np.empty((N, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    _assert_named(name, out, x)
    out.setflags(write=False)
    return out


def _band_power(z: np.ndarray, f0: float, half: float = 90e3) -> float:
    """power of z (744 187.5 S/s) within f0 +- half"""
    Z = np.fft.fft(z * np.hanning(z.size))
    f = np.fft.fftfreq(z.size, 1 / sf.FS)
    return float(np.sum(np.abs(Z[np.abs(f - f0) <= half]) ** 2))


def _assert_named(name: str, out: np.ndarray, x: np.ndarray):
    c = CASES[name]
    if name == "zero":
        assert not out.any()
        return
    if name == "fullscale":
        assert out.min() == -32768 and out.max() == 32767
        return
    assert np.abs(x.real).max() < 32767 and np.abs(x.imag).max() < 32767, name          # inside int16: nothing clips
    z = out[:, 0].astype(np.float64) + 1j * out[:, 1].astype(np.float64)
    mag = np.abs(z)
    if not c["rays"] and not c["adj"] and c["cnr"] is None:
        assert np.all(np.abs(mag - c["amp"]) < 1.0)                                     # constant amplitude: rounding only
    if name == "unmodulated":
        assert np.max(np.abs(fa.inst_freq(out))) < 1e-3
    if c["rays"] and not c["adj"] and c["cnr"] is None:                                 # the envelope moves between 1 - a and 1 + a
        a = sum(r[0] for r in c["rays"])
        assert mag.max() <= c["amp"] * (1 + a) + 1 and mag.min() >= c["amp"] * (1 - a) - 1 and mag.max() - mag.min() > 0.2 * a * c["amp"], name
    if c["adj"]:
        off, db = c["adj"]
        got = 10 * np.log10(_band_power(z, off) / _band_power(z, 0.0))
        assert abs(got - db) < (0.5 if c["cnr"] is None and not c["rays"] else 1.0), (name, got, db)     # (noise and a ray move the wanted band's power a little)
    if c["cnr"] is not None and c["cnr"] >= 20.0 and not c["rays"] and not c["adj"]:   # (below 20 dB the envelope's variance is no longer the radial half)
        got = 10 * np.log10(c["amp"] ** 2 / (2 * np.var(mag))) + cm.FILTER_GAIN_DB
        assert abs(got - c["cnr"]) < 0.5, (name, got)


@functools.lru_cache(maxsize=None)
def taps():
    """(hA, hU) as the library stores them: float32, read-only"""
    hu = im.design_hu().astype(np.float32)
    hu.setflags(write=False)
    return fa.tables()[0], hu


QUANTITIES = ("e", "eu", "du")


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """the float64 model of the input, read-only: {"e", "eu", "du", "d", "r", "t", "err32": {"e", "eu", "du": float, "t": [NS]}, "reports"}"""
    ha, hu = taps()
    m64, m32 = im.front(host(name), ha, hu), im.front(host(name), ha, hu, dtype=np.float32)
    nb = m64["t"].shape[0]
    err = {q: float(np.max(np.abs(m32[q][:nb * im.BLOCK].astype(np.float64) - m64[q][:nb * im.BLOCK]))) for q in QUANTITIES}
    err["t"] = np.max(np.abs(m32["t"] - m64["t"]), axis=0)
    info = {**m64, "err32": err, "reports": im.reports(m64["t"])}
    for v in info.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return info


def expected(name: str) -> dict:
    """what the name promises of the verdict; a key that is missing is not promised.
    multipath: a ray of a >= 0.3 raises it; the weak ray (a = 0.1, 3 us) does not -- the envelope |1 + a exp(j theta)| ~ 1 + a cos(theta) moves with
    theta = phi - 2 pi f tau, and over the +-41 kHz this programme swings that is a 0.1 sin(0.5) 0.55 ~ 0.03 rms: below depth_min = 0.05 by the
    threshold's design, a weak echo is not a verdict; without a ray it is never raised.
    adjacent / side: raised with the right side by every neighbour without added noise, never raised without neighbour and ray; under a ray alone
    (the fading itself puts e and d in step around 100 .. 170 kHz) and for the neighbour under 20 dB noise (noise dominates) nothing is promised"""
    c = CASES[name]
    out = {"multipath": any(r[0] >= 0.3 for r in c["rays"])}
    if name in ADJ_QUIET:
        out.update(adjacent=True, side=1 if c["adj"][0] > 0 else -1)
    elif name in PLAIN_CASES:
        out.update(adjacent=False, side=0)
    return out


@functools.lru_cache(maxsize=None)
def analyse(name: str) -> dict:
    """the float64 model's windowed report of the last audio block (33 blocks behind the start of the stream, where the channel filter's turn-on
    no longer weighs), asserted to show what the input is named for -> that report"""
    w = reference(name)["reports"]["windowed"]
    c = CASES[name]
    if c["rays"]:
        assert w["explained"] >= 0.7, (name, w["explained"])
    else:
        assert w["explained"] <= 0.1, (name, w["explained"])
    if name in ADJ_QUIET:
        assert abs(w["rho"]) >= 0.55 and (w["rho"] > 0) == (c["adj"][0] > 0), (name, w["rho"])
    if name in PLAIN_CASES:
        assert abs(w["rho"]) <= 0.1, (name, w["rho"])
    want = expected(name)
    assert {k: w[k] for k in want} == want, (name, w, want)
    return w


def stack(names) -> np.ndarray:
    return np.stack([host(n) for n in names])
