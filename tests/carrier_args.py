"""Seeded inputs of the carrier-measurement tests (tests/carrier_checks.py): cs16 hosts at 744 187.5 S/s, each asserted to hold what it is named
for, with the float64 model's output (tests/carrier_model.py) computed once per input and shared.  A session is fm_args.N = 120 000 input
samples: 111 blocks, 95 audio blocks."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import carrier_model as cm, fm_args as fa, fm_model as fm

N = fa.N
AMP = fa.AMP
STEREO = dict(left=[(1000.0, 0.8)], right=[(3000.0, 0.8, 1.0)])
LOUD = dict(left=[(10000.0, 0.9)], right=[(10000.0, 0.9)], pilot=None)

# name -> (programme (mpx_terms arguments) or None for no carrier, amplitude, cnr_db over the whole band or None, carrier shift Hz, seed)
CASES = {
    "silent": (dict(pilot=None), AMP, None, 0.0, 0),
    "silent5": (dict(pilot=None), AMP, 5.0, 0.0, 5),
    "silent15": (dict(pilot=None), AMP, 15.0, 0.0, 15),
    "silent35": (dict(pilot=None), AMP, 35.0, 0.0, 35),
    "stereo25": (STEREO, AMP, 25.0, 0.0, 25),
    "loud25": (LOUD, AMP, 25.0, 0.0, 26),
    "shift+1k5": (dict(pilot=None), AMP, None, 1500.0, 0),
    "shift-1k5": (dict(pilot=None), AMP, None, -1500.0, 0),
    "shift+20k": (dict(pilot=None), AMP, None, 20000.0, 0),
    "shift-20k": (dict(pilot=None), AMP, None, -20000.0, 0),
    "noise": (None, 2000.0, None, 0.0, 77),                    # complex Gaussian noise alone, 2000 rms per component
    "zero": (None, 0.0, None, 0.0, 0),
    "fullscale": (dict(left=[(1000.0, 0.3)], right=[(2500.0, 0.2)], preemph_us=75), 40000.0, None, 0.0, 0),
}
CNR_CASES = {"silent5": 5.0, "silent15": 15.0, "silent35": 35.0}      # in-filter 10.3, 20.3 and 40.3 dB
SHIFT_CASES = {k: v[3] for k, v in CASES.items() if v[3] != 0.0}
MULTI = {1: ["stereo25"], 3: ["silent15", "noise", "shift+1k5"],
         9: ["silent", "silent5", "stereo25", "loud25", "shift-20k", "noise", "zero", "fullscale", "silent35"]}


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """int16 [N, 2], read-only"""
    prog, amp, cnr, shift, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if prog is None:
        x = amp * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    else:
        terms = sf.mpx_terms(prog.get("left", ()), prog.get("right", ()), prog.get("pilot", 0.1), 0.0, 0.3, prog.get("preemph_us"))
        x = amp * np.exp(1j * (sf.fm_phase(N, terms) + 2 * np.pi * shift * np.arange(N) / sf.FS))
        if cnr is not None:
            s = amp * 10 ** (-cnr / 20) / np.sqrt(2)
            x = x + s * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    out = np.empty((N, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    _assert_named(name, out)
    out.setflags(write=False)
    return out


def _assert_named(name: str, x: np.ndarray):
    prog, amp, cnr, shift, _ = CASES[name]
    mag = np.hypot(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64))
    if name == "zero":
        assert not x.any()
    elif name == "fullscale":
        assert x.min() == -32768 and x.max() == 32767
    elif prog is None:
        assert abs(np.sqrt(np.mean(mag ** 2) / 2) / amp - 1) < 0.02 and abs(np.mean(x)) < 20          # no carrier: the mean is zero
    elif cnr is None:
        assert np.all(np.abs(mag - amp) < 1.0)                                  # constant amplitude: rounding only
        f = np.mean(fa.inst_freq(x)) * sf.DEV_HZ
        assert abs(f - shift) < 1.0, (name, f)
    else:
        got = 10 * np.log10(amp ** 2 / (2 * np.var(mag)))                       # the radial half of the noise power
        assert abs(got - cnr) < 0.5, (name, got)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """the float64 model of the input, read-only: {"r", "d", "t", "r_err32", "t_err32" [3], "reports"}"""
    ha = fa.tables()[0]
    r, d, t = cm.front(host(name), ha)
    r32, _, t32 = cm.front(host(name), ha, dtype=np.float32)
    info = {"r": r, "d": d, "t": t, "r_err32": float(np.max(np.abs(r32.astype(np.float64) - r))),
            "t_err32": np.max(np.abs(t32 - t), axis=0), "reports": cm.reports(t)}
    for v in info.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return info


def stack(names) -> np.ndarray:
    return np.stack([host(n) for n in names])


def ha_noise_gain_db() -> float:
    """10 log10(sum hA^2): what the channel filter leaves of white noise"""
    h = fm.design_ha()
    return float(10 * np.log10(np.sum(h * h)))
