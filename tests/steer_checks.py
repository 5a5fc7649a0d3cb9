"""The checks of reception steering (nrsc5hip_fm_steer*, k_fm_audio<true> in nrsc5_amd/csrc/k_fm_audio.hip), written once and run twice: by
tests/test_steer_stage_cpu.py on the CPU-emulated twin and by tests/test_gpu_steer_stage.py on gfx950.  The reference is the float64 restatement
tests/steer_model.py on the inputs of tests/steer_args.py.

Bounds.  (q, b, h, g) through the stage hook: 4 x the largest |float32 model - float64 model| of the same input and quantity (the rule of
carrier_checks.check_stage_sums); where both models sit on a clamp that bound is 0 and the library has to sit on it too, which
steer_args.analyse makes safe: the clamped inputs are at least 100 bounds away from the thresholds.  Audio: the rule of fm_checks.compare, no
sample more than 1 LSB from the float64 model, at most 1 % of the samples different, the clip counts equal; once against the model with its own
factors and once against the model mixing with the library's factors.  The exact properties are byte comparisons."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import carrier_checks as cc, fm_checks as fc, fm_model as fm, steer_args as sa, steer_model as sm

S0 = fm.BLOCK_OUT * sa.SETTLED                 # the first frame of audio block 18
push = cc.push


def gains_of(names):
    return [sa.GAINS.get(n, 1.0) for n in names]


def steered(be: fc.Backend, names, cfg=None, **kw):
    return be.demod(len(names), gains=gains_of(names), steer=dict(cfg) if cfg else True, **kw)


def run(be: fc.Backend, names, cfg=None, steer=True, chunks=(), **kw):
    """-> (pcm [K, frames, 2], clips [K, 2], steer() or None)"""
    D = steered(be, names, cfg, **kw) if steer else be.demod(len(names), gains=gains_of(names), **kw)
    pcm = push(be, D, sa.stack(names), list(chunks))
    out = pcm, D.clip_counts(), (D.steer() if steer else None)
    D.close()
    return out


def stage(be: fc.Backend, names, cfg=None) -> np.ndarray:
    D = steered(be, names, cfg)
    keep, ptr = be.upload(sa.stack(names))
    fac = D.stage_steer(ptr, 2 * sa.N, sa.N)
    D.close()
    return fac


def compare(got: np.ndarray, clips, want: np.ndarray, want_clips, what) -> float:
    """the rule of fm_checks.compare -> the share of samples that differ"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float(np.mean(diff != 0)) if diff.size else 0.0
    print(f"{what}: largest difference {diff.max() if diff.size else 0} LSB, {100 * share:.4f} % of the samples differ, clips {list(clips)}")
    assert diff.max() <= 1, (what, diff.max())
    assert share <= 0.01, (what, share)
    assert np.array_equal(np.asarray(clips), want_clips), (what, clips, want_clips)
    return share


# ----------------------------------------------------------------------------------------------------- 1. factors (stage hook)
def check_factors(be: fc.Backend, names=None) -> list:
    """-> the lines of profiles/wideband_steer_cases.txt"""
    sa.analyse()
    names = list(names or sa.CASES)
    fac = stage(be, names)
    assert fac.shape == (len(names), 95, 4)
    lines = []
    for c, name in enumerate(names):
        info = sa.reference(name)[2]
        err = np.max(np.abs(fac[c].astype(np.float64) - info["factors"]), axis=0)
        bound = 4 * info["fac_err32"]
        lines.append(f"{name:10s} " + "  ".join(f"{k} {e:.3g} (bound {b:.3g})" for k, e, b in zip("qbhg", err, bound)))
        print(lines[-1])
        assert np.all(np.isfinite(fac[c])) and np.all((fac[c] >= 0) & (fac[c] <= 1))
        assert np.all(err <= bound), (name, err, bound)
    by = dict(zip(names, fac))
    for name, sign in (("fade_up", 1.0), ("fade_down", -1.0)):
        if name in by:
            assert np.all(sign * np.diff(by[name][:, :3], axis=0) >= 0), name
    if "clean" in by:                                           # c_j: the start of a session is not read as bad reception
        want = sa.reference("clean")[2]["factors"]
        assert np.all(np.abs(by["clean"][:18, 1] - want[:18, 1]) <= 4 * sa.reference("clean")[2]["fac_err32"][1])
        assert np.all(by["clean"][1:18, 1] > 0.5) and np.all(by["clean"][1:18, 0] > 0.99)      # with the constant 17, block 1 would read q = 0.30
    return lines


# ---------------------------------------------------------------------------------------------------- 2. audio against the model
def check_audio(be: fc.Backend, name: str) -> tuple:
    """-> (share end to end, share with the library's factors)"""
    sa.analyse()
    pcm, clips, _ = run(be, [name])
    want, want_clips, info = sa.reference(name)
    a = compare(pcm[0], clips[0], want, want_clips, f"{name} end to end (float32 model {100 * info['share32']:.4f} %)")
    fac = stage(be, [name])[0]
    want, want_clips = sa.with_factors(name, fac)
    b = compare(pcm[0], clips[0], want, want_clips, f"{name} mixing alone")
    return a, b


def shares_report(be: fc.Backend) -> list:
    lines = []
    for name in sa.CASES:
        a, b = check_audio(be, name)
        ref = sa.reference(name)
        lines.append(f"{name:10s} differing {100 * a:.4f} % end to end, {100 * b:.4f} % with the library's factors;  float32 model {100 * ref[2]['share32']:.4f} %  "
                     f"rms {np.sqrt(np.mean(ref[0].astype(np.float64) ** 2)):7.0f} LSB")
    return lines


# ------------------------------------------------------------------------------------------------------- 3. exact properties
def check_exact(be: fc.Backend):
    sa.analyse()
    names = ["clean", "cnr24", "cnr15", "cnr6", "cnr0", "noise", "zero"]
    plain, plain_clips, _ = run(be, names, steer=False)
    got, clips, last = run(be, names)
    by, un = dict(zip(names, got)), dict(zip(names, plain))
    assert by["clean"][S0:].tobytes() == un["clean"][S0:].tobytes() and un["clean"][S0:].any()      # above every ramp: the unsteered bytes
    assert by["clean"][:S0].tobytes() != un["clean"][:S0].tobytes()                                 # (the turn-on in block 0 reads about 25 dB)
    for name in ("cnr0", "cnr6"):                                                                     # below the blend ramp: L == R
        assert np.array_equal(by[name][S0:, 0], by[name][S0:, 1]) and not np.array_equal(un[name][S0:, 0], un[name][S0:, 1]), name
    assert not by["zero"].any() and not un["zero"].any()
    floor = np.float32(10.0 ** (-20.0 / 20.0))
    fac = stage(be, ["noise"])[0]
    assert not fac[:, 1].any() and not fac[:, 2].any() and np.all(fac[:, 3] == floor), fac[:, 1:].max(axis=0)
    given = np.tile(np.array([0.0, 0.0, 0.0, floor], dtype=np.float32), (95, 1))
    want, want_clips = sa.with_factors("noise", given)
    compare(by["noise"], clips[names.index("noise")], want, want_clips, "noise at the floor")
    assert last[names.index("noise")]["mute"] == floor and last[0] == {"q": last[0]["q"], "blend": 1.0, "highcut": 1.0, "mute": 1.0}
    # controls = 0: the unsteered bytes everywhere
    off, off_clips, _ = run(be, names, cfg=dict(controls=0))
    assert off.tobytes() == plain.tobytes() and np.array_equal(off_clips, plain_clips)
    # each control alone
    blend, blend_clips, _ = run(be, names, cfg=dict(controls=sm.BLEND))
    highcut, highcut_clips, _ = run(be, names, cfg=dict(controls=sm.HIGHCUT))
    mute, mute_clips, _ = run(be, names, cfg=dict(controls=sm.MUTE))
    i6, i15, i24 = names.index("cnr6"), names.index("cnr15"), names.index("cnr24")
    assert np.array_equal(blend[i6][S0:, 0], blend[i6][S0:, 1])                                       # blend alone: mono at 6 dB ...
    assert mute[i15].tobytes() == plain[i15].tobytes()                                                # mute alone at 15 dB: nothing to do
    assert highcut[i24][S0:].tobytes() == plain[i24][S0:].tobytes()                                   # high-cut alone at 24 dB: the wide table
    assert not np.array_equal(highcut[i6][S0:, 0], highcut[i6][S0:, 1]) and highcut[i6][S0:].tobytes() != plain[i6][S0:].tobytes()   # ... and stereo stays
    assert not np.array_equal(mute[i6][S0:, 0], mute[i6][S0:, 1]) and np.abs(mute[i6][S0:]).max() < np.abs(plain[i6][S0:]).max()
    for cfg, out, out_clips in ((dict(controls=sm.BLEND), blend, blend_clips), (dict(controls=sm.HIGHCUT), highcut, highcut_clips), (dict(controls=sm.MUTE), mute, mute_clips)):
        for i in (i6, i15, i24):
            want, want_clips, _ = sa.reference(names[i], cfg)
            compare(out[i], out_clips[i], want, want_clips, f"{names[i]} controls {cfg['controls']}")


# ----------------------------------------------------------------------------------------------------------- 4. narrow table
def check_narrow_table(be: fc.Backend):
    for de in (75.0, 50.0, 0.0):
        P = be.demod(1, deemphasis_us=de)
        D = be.demod(1, deemphasis_us=de, steer=True)
        tab = D.steer_taps()
        assert (D.taps_audio, D.phases, D.taps_channel) == (P.taps_audio, P.phases, P.taps_channel) and tab.shape == (fm.PHASES, D.taps_audio)
        assert D.tables()[1].tobytes() == P.tables()[1].tobytes()                  # the wide table is what it was
        P.close(); D.close()
        assert np.max(np.abs(tab.astype(np.float64) - sm.design_narrow(de))) <= 2.0 ** -24 * np.max(np.abs(tab))
        g = fm.prototype(tab)
        nfft = 1 << 19
        H = np.abs(np.fft.rfft(g, nfft))
        fr = np.arange(H.size) * (fm.PHASES * fm.FS1) / nfft
        db = 20 * np.log10(np.maximum(H / H[0], 1e-30))
        want = -10 * np.log10(1 + (2 * np.pi * fr * de * 1e-6) ** 2)
        pb = fr <= sm.PASS_N
        assert pb.sum() > 300 and np.max(np.abs(db[pb] - want[pb])) <= 0.1, np.max(np.abs(db[pb] - want[pb]))
        assert np.max(db[fr >= sm.STOP_N]) <= -60.0, np.max(db[fr >= sm.STOP_N])
        assert abs(g.sum() - fm.PHASES) < 1e-4
        print(f"deemphasis {de:g}: narrow table {tab.shape[1]} taps x 16, passband error {np.max(np.abs(db[pb] - want[pb])):.4f} dB to 4 kHz, "
              f"stopband {np.max(db[fr >= sm.STOP_N]):.1f} dB from 8 kHz")


# --------------------------------------------------------------------------------------------------------------- 5. physical
PHYS_CFG = dict(highcut_db=(20.0, 30.0))       # at 15 dB: h = 0 as well as b = 0
BAND = (8000.0, 15000.0)                       # "above 8 kHz": up to the wide table's pass edge; beyond it both tables are in their stop band


def _band_power(y: np.ndarray) -> float:
    """power of y (44.1 kS/s) inside BAND under a Hann window"""
    n = y.size
    Y = np.fft.rfft(y * (0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)))
    f = np.arange(Y.size) * fm.AUDIO_RATE / n
    return float(np.sum(np.abs(Y[(f >= BAND[0]) & (f <= BAND[1])]) ** 2))


def predicted_fall() -> float:
    """what the two tables' responses predict for the noise power inside BAND, narrow over wide, as a ratio: the resampler is the prototype H
    at 16 Fs1 between d repeated every Fs1 and a decimation to 44.1 kS/s, so the output's spectrum at f is the sum over k of
    |H(f + 44100 k)|^2 Sd((f + 44100 k) mod Fs1), Sd the spectrum of the discriminator's noise (the model's d of the noisy input less that of the
    clean one, averaged periodograms).  The images count: an FM discriminator's noise rises with frequency far beyond the audio band, and what
    the stop band leaves of it comes on top of what the response leaves of the noise inside BAND itself (with the de-emphasis in the prototype
    the stop bands are 85 dB and more, and the images stay small)"""
    ha, tab, tab_n = sa.tables()
    nd = (fm.front(sa.host("cnr15"), ha.astype(np.float64))[0] - fm.front(sa.host("clean"), ha.astype(np.float64))[0])[fm.BLOCK * sa.SETTLED:]
    seg = 8192
    win = np.hanning(seg)
    Sd = np.mean([np.abs(np.fft.rfft(nd[i:i + seg] * win)) ** 2 for i in range(0, nd.size - seg + 1, seg // 2)], axis=0)
    fd = np.arange(Sd.size) * fm.FS1 / seg
    n = 1 << 19
    fgrid = np.arange(n // 2 + 1) * (fm.PHASES * fm.FS1) / n
    f = np.arange(BAND[0], BAND[1] + 1.0, 25.0)
    out = []
    for t in (tab_n, tab):
        H2 = np.abs(np.fft.rfft(fm.prototype(t), n)) ** 2
        total = 0.0
        for k in range(-68, 69):
            F = np.abs(f + fm.AUDIO_RATE * k)
            fold = np.mod(F, fm.FS1)
            fold = np.minimum(fold, fm.FS1 - fold)
            total += float(np.sum(np.where(F < fgrid[-1], np.interp(F, fgrid, H2) * np.interp(fold, fd, Sd), 0.0)))
        out.append(total)
    return out[0] / out[1]


def physical(steered_pcm: np.ndarray, plain_pcm: np.ndarray, who: str):
    """noise = output less the model's audio of the clean programme under the same controls (the library's own factors are 0, 0, 1 from block 17
    on, as the model's are: check_physical asserts it)"""
    given = sa.reference("cnr15", PHYS_CFG)[2]["factors"].astype(np.float32)
    clean_s = sa.with_factors("clean", given, PHYS_CFG)[0].astype(np.float64)
    clean_u = sa.reference("clean", dict(controls=0))[0].astype(np.float64)
    assert np.array_equal(steered_pcm[S0:, 0], steered_pcm[S0:, 1])                # b = 0: no noise in L - R at all
    ms, mu, cs, cu = (v[S0:].astype(np.float64).mean(axis=1) for v in (steered_pcm, plain_pcm, clean_s, clean_u))
    # the int16 rounding of the steered output and of its clean audio (L == R in both: one rounding each): 2 / 12 LSB^2
    floor = 2.0 * _band_power(np.random.default_rng(0).uniform(-0.5, 0.5, ms.size))
    before = _band_power(mu - cu)
    got, want = _band_power(ms - cs), before * predicted_fall() + floor
    fall, fall_want = 10 * np.log10(got / before), 10 * np.log10(want / before)
    tones = [20 * np.log10(fm.tone(ms, f, 0) / fm.tone(mu, f, 0)) for f in (1000.0, 3000.0)]
    print(f"{who}: noise from 8 to 15 kHz falls by {-fall:.2f} dB (the tables' responses and the rounding floor predict {-fall_want:.2f} dB); tones at 1 / 3 kHz "
          f"move by {tones[0]:+.3f} / {tones[1]:+.3f} dB")
    assert abs(fall - fall_want) <= 1.0, (who, fall, fall_want)
    assert fall < -20.0, (who, fall)
    assert all(abs(t) <= 0.1 for t in tones), (who, tones)


def check_physical(be: fc.Backend):
    f = sa.reference("cnr15", PHYS_CFG)[2]["factors"][sa.SETTLED - 1:]
    assert not f[:, 1].any() and not f[:, 2].any() and np.all(f[:, 3] == 1.0)
    physical(sa.reference("cnr15", PHYS_CFG)[0], sa.reference("cnr15", dict(controls=0))[0], "model")      # the definition first, on the CPU
    got, _, _ = run(be, ["cnr15"], cfg=PHYS_CFG)
    plain, _, _ = run(be, ["cnr15"], steer=False)
    physical(got[0], plain[0], "library")


# --------------------------------------------------------------------------------------------------------------- 6. chunking
CHUNK_NAMES, CHUNK_GAINS = ["clean", "fade_down", "noise"], [1.5, 1.0, 1.0]


def check_chunking(be: fc.Backend, plans=None):
    """three channels, the first one clipping: every chunking gives the bytes, factors, carrier report and clip counts of the single push"""
    x = sa.stack(CHUNK_NAMES)
    D = be.demod(3, gains=CHUNK_GAINS, steer=True)
    ref_pcm = push(be, D, x, [])
    ref = (D.steer(), D.carrier(), D.clip_counts().tobytes())
    assert D.clip_counts()[0].sum() > 0
    fac = stage(be, CHUNK_NAMES)
    for c in range(3):
        assert list(ref[0][c].values()) == [float(v) for v in fac[c, -1]], (c, ref[0][c], fac[c, -1])
    all_plans = fc.chunk_plans(sa.N)
    for plan in plans or all_plans:
        D.reset()
        sizes = all_plans[plan]
        stride = 1 if len(sizes) < 500 else 97
        count = [0]

        def look(pos):
            count[0] += 1
            if count[0] % stride and pos != sa.N:
                return
            a = max(0, ((pos + 1) // 2) // fm.BLOCK - fm.W)
            got = D.steer()
            for c in range(3):                                  # after every look: the factors of the last block delivered so far
                want = [float(v) for v in fac[c, a - 1]] if a else [0.0] * 4
                assert list(got[c].values()) == want, (plan, pos, c, got[c], want)

        pcm = push(be, D, x, sizes, look)
        assert pcm.tobytes() == ref_pcm.tobytes(), plan
        assert (D.steer(), D.carrier(), D.clip_counts().tobytes()) == ref, plan
    D.close()


# --------------------------------------------------------------------------------------------------------------- 7. channels
def check_channels(be: fc.Backend, k: int):
    names = sa.MULTI[k]
    pcm, clips, last = run(be, names, chunks=[33333])
    for c, name in enumerate(names):
        one, one_clips, one_last = run(be, [name])
        assert pcm[c].tobytes() == one[0].tobytes() and np.array_equal(clips[c], one_clips[0]) and last[c] == one_last[0], (k, name)


# ------------------------------------------------------------------------------------------------------------- 8. life cycle
def check_life_cycle(be: fc.Backend):
    names = ["cnr24", "cnr6"]
    x = sa.stack(names)
    n = sa.N
    D = be.demod(2)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # unsteered: refused
        D.steer()
    assert ei.value.code == eng.EINVAL and "not enabled" in str(ei.value)
    keep_in, p_in = be.upload(x)
    cap = fm.outputs_total(n)
    keep_out, p_out = be.zeros((2, cap, 2))
    D.process(p_in, 2 * n, 1000, p_out, 2 * cap, cap)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # after a push: refused
        D.steer_enable()
    assert ei.value.code == eng.EINVAL and "before the first push" in str(ei.value)
    D.close()
    D = be.demod(2, steer=True)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # twice: refused
        D.steer_enable()
    assert ei.value.code == eng.EINVAL and "already" in str(ei.value)
    assert all(v == {"q": 0.0, "blend": 0.0, "highcut": 0.0, "mute": 0.0} for v in D.steer())      # nothing delivered yet
    first_pcm = push(be, D, x, [33333])
    first = (D.steer(), D.carrier(), D.clip_counts().tobytes())
    assert 0.0 < first[0][0]["blend"] < 1.0 and first[0][1]["blend"] == 0.0 and 0.1 < first[0][1]["mute"] < 1.0
    D.reset()                                                   # still steered, the snapshot zero
    assert all(not any(v.values()) for v in D.steer())
    second_pcm = push(be, D, x, [])
    assert second_pcm.tobytes() == first_pcm.tobytes() and (D.steer(), D.carrier(), D.clip_counts().tobytes()) == first
    D.close()
    bad = [dict(blend_db=(30.0, 18.0)), dict(highcut_db=(10.0, 10.0)), dict(mute_db=(2.0, float("nan"))), dict(mute_db=(float("-inf"), 8.0)),
           dict(blend_db=(18.0, float("inf"))), dict(mute_floor_db=1.0), dict(mute_floor_db=float("nan")), dict(controls=8)]
    for kw in bad:
        with pytest.raises(eng.Nrsc5HipError) as ei:
            be.demod(1, steer=kw)
        assert ei.value.code == eng.EINVAL, kw
    # with the carrier measurement already on; and the report of a steered object is the carrier-only object's, bit for bit
    C = be.demod(2, carrier=True)
    push(be, C, x, [33333])
    only = C.carrier()
    C.close()
    B = be.demod(2, carrier=True, steer=True)
    both_pcm = push(be, B, x, [7777])
    assert both_pcm.tobytes() == first_pcm.tobytes() and B.carrier() == only == first[1] and B.steer() == first[0]
    B.close()


# ----------------------------------------------------------------------------------------------------------- 9. launch counts
def check_launch_counts(be: fc.Backend):
    x = sa.stack(["cnr15"])
    sizes = [1081] * 40 + [1] * 5 + [50000]
    count = {}
    for kind, kw in (("plain", {}), ("carrier", dict(carrier=True)), ("steer", dict(steer=True))):
        D = be.demod(1, **kw)
        keep, ptr = be.upload(x)
        if kind == "steer":
            D.stage_steer(ptr, 2 * sa.N, sa.N)                  # the stage hook is not counted
        push(be, D, x, sizes)
        count[kind] = D.launches()
        D.close()
    assert count["plain"] == cc.launches_expected(sizes, sa.N), count
    assert count["steer"] == count["carrier"] > count["plain"], count
