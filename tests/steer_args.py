"""Seeded inputs of the reception-steering tests (tests/steer_checks.py): cs16 hosts at 744 187.5 S/s from nrsc5_amd/synth_fm.py and seeded complex
Gaussian noise, as tests/carrier_args.py builds them, with the float64 model's output (tests/steer_model.py) computed once per input and
configuration and shared.  A session is fm_args.N = 120 000 input samples: 111 blocks, 95 audio blocks.

CNR here is the figure the thresholds are written in: in the channel filter's noise bandwidth, carrier_model.FILTER_GAIN_DB above the CNR over the
whole sampled band.  A fade is a noise amplitude that moves linearly over the session between the amplitudes of its two CNRs."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import carrier_model as cm, fm_args as fa, fm_model as fm, steer_model as sm

N = fa.N
AMP = fa.AMP
STEREO = dict(left=[(1000.0, 0.8)], right=[(3000.0, 0.8, 1.0)])
MONO = dict(left=[(1000.0, 0.3)], right=[(1000.0, 0.3)], pilot=None, preemph_us=75)
SETTLED = 18                                   # audio blocks from which on the exact properties are stated (block 0 holds the channel filter's turn-on)

# name -> (programme or None for no carrier, amplitude, CNR dB: a figure, a (from, to) fade or None, seed)
CASES = {
    "clean": (STEREO, AMP, None, 0),
    "cnr24": (STEREO, AMP, 24.0, 24),
    "cnr15": (STEREO, AMP, 15.0, 15),
    "cnr6": (STEREO, AMP, 6.0, 6),
    "cnr0": (STEREO, AMP, 0.0, 100),
    "fade_down": (STEREO, AMP, (35.0, 0.0), 350),
    "fade_up": (STEREO, AMP, (0.0, 35.0), 35),
    "noise": (None, 2000.0, None, 77),
    "zero": (None, 0.0, None, 0),
    "clipping": (dict(left=[(1000.0, 0.3)], right=[(2500.0, 0.2)], preemph_us=75), 40000.0, None, 0),
    "mono15": (MONO, AMP, 15.0, 115),
}
GAINS = {"clipping": 2.0}      # the audio clips on the peaks; at 4 the float32 model alone passes 0.5 %
MULTI = {1: ["cnr15"], 3: ["clean", "fade_down", "noise"], 9: ["clean", "cnr24", "cnr15", "cnr6", "cnr0", "fade_up", "noise", "zero", "mono15"]}
F32_SHARE_MAX = 0.005


def _noise_amp(amp: float, cnr_db: float) -> float:
    """rms per component of white noise that leaves cnr_db in the channel filter's bandwidth"""
    return amp * 10 ** (-(cnr_db - cm.FILTER_GAIN_DB) / 20) / np.sqrt(2)


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """int16 [N, 2], read-only"""
    prog, amp, cnr, seed = CASES[name]
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    if prog is None:
        x = amp * w
    else:
        terms = sf.mpx_terms(prog.get("left", ()), prog.get("right", ()), prog.get("pilot", 0.1), 0.0, 0.3, prog.get("preemph_us"))
        x = amp * np.exp(1j * sf.fm_phase(N, terms))
        if isinstance(cnr, tuple):
            x = x + np.linspace(_noise_amp(amp, cnr[0]), _noise_amp(amp, cnr[1]), N) * w
        elif cnr is not None:
            x = x + _noise_amp(amp, cnr) * w
    out = np.empty((N, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    if name == "zero":
        assert not out.any()
    if name == "clipping":
        assert out.min() == -32768 and out.max() == 32767
    out.setflags(write=False)
    return out


def stack(names) -> np.ndarray:
    return np.stack([host(n) for n in names])


@functools.lru_cache(maxsize=None)
def tables(deemphasis_us: float = 75.0):
    """(ha, wide, narrow) rounded to float32 as the library stores them"""
    ha, tab = fa.tables(deemphasis_us)
    tab_n = sm.design_narrow(deemphasis_us).astype(np.float32)
    tab_n.setflags(write=False)
    return ha, tab, tab_n


def _key(cfg: dict | None):
    cfg = sm.config(**(cfg or {}))
    return tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in cfg.items()))


@functools.lru_cache(maxsize=None)
def _reference(name: str, key, gain: float):
    cfg = dict(key)
    ha, tab, tab_n = tables()
    pcm, clips, info = sm.model(host(name), ha, tab, tab_n, cfg, gain=gain)
    pcm32, _, info32 = sm.model(host(name), ha, tab, tab_n, cfg, gain=gain, dtype=np.float32)
    diff = np.abs(pcm.astype(np.int32) - pcm32.astype(np.int32))
    info["share32"] = float(np.mean(diff != 0)) if diff.size else 0.0
    info["max32"] = int(diff.max()) if diff.size else 0
    info["fac_err32"] = np.max(np.abs(info32["factors"].astype(np.float64) - info["factors"]), axis=0)       # [4]: q, b, h, g
    pcm.setflags(write=False)
    for v in info.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pcm, clips, info


def reference(name: str, cfg: dict | None = None, gain: float | None = None):
    """-> (pcm int16 [frames, 2], clips [2], info) of the float64 model, read-only; info also holds "share32", "max32" and "fac_err32", the float32
    model's distance"""
    return _reference(name, _key(cfg), GAINS.get(name, 1.0) if gain is None else gain)


def with_factors(name: str, given: np.ndarray, cfg: dict | None = None, gain: float | None = None):
    """the float64 model mixing with the given (q, b, h, g) per block -> (pcm, clips)"""
    ha, tab, tab_n = tables()
    pcm, clips, _ = sm.model(host(name), ha, tab, tab_n, sm.config(**(cfg or {})), gain=GAINS.get(name, 1.0) if gain is None else gain, given=given)
    return pcm, clips


def thresholds(cfg: dict | None = None):
    """-> (the largest q_hi, the smallest q_lo) over the three ramps"""
    cfg = sm.config(**(cfg or {}))
    pairs = [cfg["blend_db"], cfg["highcut_db"], cfg["mute_db"]]
    return max(sm.q_of_db(p[1]) for p in pairs), min(sm.q_of_db(p[0]) for p in pairs)


@functools.lru_cache(maxsize=None)
def analyse() -> dict:
    """what the tests take for granted about the inputs, asserted once on the CPU with the defaults: the float32 model's share, the clamped inputs
    away from the thresholds, the fades monotonic in the model, the named CNRs -> name -> {"share32", "fac_err32", "q_min", "q_max"}"""
    q_hi, q_lo = thresholds()
    out = {}
    for name in CASES:
        _, _, info = reference(name)
        assert info["max32"] <= 1 and info["share32"] <= F32_SHARE_MAX, (name, info["max32"], info["share32"])
        q = info["q"][SETTLED:]
        bound = 4 * info["fac_err32"][0]
        out[name] = {"share32": info["share32"], "fac_err32": info["fac_err32"], "q_min": float(q.min()), "q_max": float(q.max())}
        if name == "clean":
            assert q.min() - q_hi >= 100 * bound, (name, q.min(), q_hi, bound)
        if name in ("cnr0", "noise"):
            assert q_lo - q.max() >= 100 * bound, (name, q.max(), q_lo, bound)
        if isinstance(CASES[name][2], float):                 # the named CNR, by the estimator's own formula, at the end of the session
            u = np.sqrt(max(q[-1], 1e-12))
            got = 10 * np.log10(u / (1 - u))
            assert abs(got - CASES[name][2]) < 1.0, (name, got)
    for name, sign in (("fade_up", 1.0), ("fade_down", -1.0)):
        fac = reference(name)[2]["factors"]
        assert np.all(sign * np.diff(fac[:, :3], axis=0) >= 0), name
    f6, f0 = reference("cnr6")[2]["factors"][SETTLED:], reference("cnr0")[2]["factors"][SETTLED:]
    assert not f6[:, 1].any() and not f0[:, 1].any()           # below the blend ramp: mono
    f15 = reference("cnr15")[2]["factors"][SETTLED:]
    assert np.all(f15[:, 3] == 1.0) and not f15[:, 1].any() and np.all((f15[:, 2] > 0) & (f15[:, 2] < 1))
    return out
