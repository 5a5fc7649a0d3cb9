"""The checks of the reception impairments (nrsc5hip_fm_impair*, nrsc5_amd/csrc/k_fm_impair.hip), written once and run twice: by
tests/test_impair_stage_cpu.py on the CPU-emulated twin and by tests/test_gpu_impair_stage.py on gfx950.  The reference is the float64
restatement tests/impair_model.py on the inputs of tests/impair_args.py, whose analyse() asserts on that model what each input is named for.

Bounds.  e, eu, du and the eleven block sums through the stage hook: 4 x the largest |float32 model - float64 model| of the same input and
quantity (the rule of the carrier measurement).  Everything with a stated order is compared bit for bit: e with the correctly rounded root of
the library's own r, the block sums with the model's sums of the library's own d, e, eu, du, the windowed and running sums with the model's
sums of the library's own block records.  The figures are the model's formula on the library's sums: explained, depth, slope, curvature and
rho use only + - x / and sqrt in a stated order and are compared bit for bit; usn_db and ripple_db go through log10, which two libm's may round
differently: 1e-9 dB.  The verdicts are judged on the windowed report of the last audio block, as analyse() does: the running report of a
111-block session still holds the channel filter's turn-on (x[n] = 0 for n < 0), a step of e and a jump of d that no later block has."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import carrier_checks as cc, fm_args as fa, fm_checks as fc, fm_model as fm, impair_args as ia, impair_model as im

DB_TOL = 1e-9
EXACT = ("explained", "depth", "slope", "curvature", "rho")
push = cc.push


def demod(be: fc.Backend, nchan: int, impair=True, **kw):
    return be.demod(nchan, impair=impair, **kw)


def stage(be: fc.Backend, names) -> dict:
    D = be.demod(len(names))                                   # the hook needs no enabled object
    keep, ptr = be.upload(ia.stack(names))
    out = D.stage_impair(ptr, 2 * ia.N, ia.N)
    out["r"], _ = D.stage_carrier(ptr, 2 * ia.N, ia.N)
    out["d"], _ = D.stage_mpx(ptr, 2 * ia.N, ia.N)
    D.close()
    return out


def assert_report(got: dict, t: np.ndarray, blocks: int, what="", cfg=None):
    """one channel's nrsc5hip_fm_impair against the model's sums of the block records t, bit for bit, and the figures by the formula"""
    want = im.reports(t[:blocks], cfg)
    assert got["blocks"] == want["blocks"] and got["audio_blocks"] == want["audio_blocks"], (what, got, want)
    for kind in ("windowed", "running"):
        g, w = got[kind], want[kind]
        for q in im.SUMS + ("count",) + EXACT + ("multipath", "adjacent", "side"):
            assert g[q] == w[q], (what, kind, q, g[q], w[q])
        for q in ("usn_db", "ripple_db"):
            assert abs(g[q] - w[q]) <= DB_TOL * max(1.0, abs(w[q])), (what, kind, q, g[q], w[q])
        assert all(np.isfinite(g[q]) for q in im.FIGURES), (what, kind, g)
        assert im.DB_MIN <= g["usn_db"] <= im.DB_MAX and im.DB_MIN <= g["ripple_db"] <= im.DB_MAX and 0.0 <= g["explained"] <= 1.0 and abs(g["rho"]) <= 1.0


# ------------------------------------------------------------------------------------ 1. e, eu, du and the block sums against the model
def check_stage(be: fc.Backend, names=None) -> list:
    """-> one line per input: the observed errors and their bounds.  The bound is the issue's rule on this one seeded input per case; the closest any
    quantity comes to it on gfx950 is Cdd of ray5us, 2.61e-7 against 2.81e-7 (93 %; every other sum at most 60 %): deterministic for a given build,
    but a compiler that pairs the fmas otherwise may move it -- if this fails there, compare the figures in profiles/wideband_impair_cases.txt first"""
    names = list(names or ia.CASES)
    got = stage(be, names)
    nb = ia.N // 2 // im.BLOCK
    assert got["e"].shape == (len(names), nb * im.BLOCK) and got["sums"].shape == (len(names), nb, im.NS)
    lines = []
    for c, name in enumerate(names):
        ref = ia.reference(name)
        err = {q: float(np.max(np.abs(got[q][c].astype(np.float64) - ref[q][:nb * im.BLOCK]))) for q in ia.QUANTITIES}
        err_t = np.max(np.abs(got["sums"][c] - ref["t"]), axis=0)
        line = f"{name}: " + "; ".join(f"{q} within {err[q]:.3g} (bound {4 * ref['err32'][q]:.3g})" for q in ia.QUANTITIES)
        line += "; block sums " + " ".join(f"{s} {err_t[i]:.3g} ({4 * ref['err32']['t'][i]:.3g})" for i, s in enumerate(im.SUMS))
        print(line)
        lines.append(line)
        assert all(np.all(np.isfinite(got[q][c])) for q in ia.QUANTITIES + ("sums",)), name
        for q in ia.QUANTITIES:
            assert err[q] <= 4 * ref["err32"][q], (name, q, err[q], 4 * ref["err32"][q])
        assert np.all(err_t <= 4 * ref["err32"]["t"]), (name, err_t, 4 * ref["err32"]["t"])
    return lines


# ------------------------------------------------------------------------------------------ 2. the stated orders, bit for bit
def check_orders(be: fc.Backend):
    names = list(ia.CASES)
    got = stage(be, names)
    nb = got["sums"].shape[1]
    for c, name in enumerate(names):
        e = im.amplitude(got["r"][c], np.float32)[:nb * im.BLOCK]             # numpy's float32 sqrt is the correctly rounded one
        assert np.array_equal(e, got["e"][c]), (name, int(np.sum(e != got["e"][c])))
        d = got["d"][c][:nb * im.BLOCK]
        assert np.array_equal(im.block_sums_in_order(d, got["e"][c], got["eu"][c], got["du"][c]), got["sums"][c]), name


# ------------------------------------------------------------------------------------ 3. 4. 5. reports, figures, verdicts, clamps
def check_report(be: fc.Backend):
    names = list(ia.CASES)
    t = stage(be, names)["sums"]
    D = demod(be, len(names))
    empty = D.impair()
    assert all(v["blocks"] == 0 and v["audio_blocks"] == 0 and not any(v["windowed"].values()) and not any(v["running"].values()) for v in empty)
    push(be, D, ia.stack(names), [50000])
    got = D.impair()
    D.close()
    for c, name in enumerate(names):
        assert_report(got[c], t[c], t.shape[1], name)
        want, w = ia.analyse(name), got[c]["windowed"]
        print(f"{name}: explained {w['explained']:.4f} depth {w['depth']:.4f} slope {w['slope']:+.3f} curvature {w['curvature']:+.3f} usn {w['usn_db']:.1f} dB "
              f"ripple {w['ripple_db']:.1f} dB rho {w['rho']:+.3f} -> multipath {w['multipath']} adjacent {w['adjacent']} side {w['side']:+d} "
              f"(model: {want['explained']:.4f} {want['depth']:.4f} {want['rho']:+.3f})")
        assert (w["multipath"], w["adjacent"], w["side"]) == (want["multipath"], want["adjacent"], want["side"]), (name, w, want)
        promised = ia.expected(name)
        assert {k: w[k] for k in promised} == promised, (name, w, promised)
    by = dict(zip(names, got))
    for kind in ("windowed", "running"):
        z = by["zero"][kind]
        assert all(z[q] == 0.0 for q in EXACT) and z["usn_db"] == im.DB_MIN and z["ripple_db"] == im.DB_MIN and not z["multipath"] and not z["adjacent"] and z["side"] == 0
    u = by["unmodulated"]["windowed"]                           # no frequency to fit against: the singular system
    assert u["explained"] == 0.0 and u["depth"] == 0.0 and u["slope"] == 0.0 and u["curvature"] == 0.0 and not u["multipath"]


# ----------------------------------------------------------------------------------------------------------------------- 6. chunking
CHUNK_NAMES = ["ray5us", "adj+200_+10", "fullscale"]


def chunk_plans(n: int) -> dict:
    """the analog FM tests' plans (pushes of 7, 1079, 1080, 1081 samples, random sizes, 3000 pushes of one sample) and seven equal pushes"""
    return {**fc.chunk_plans(n), "seven_pushes": [n // 7 + 1] * 7}


def check_chunking(be: fc.Backend, plans=None):
    """after every look the reports equal the model's sums of the whole session's block records up to the blocks complete by then, so every
    chunking gives the bits of the single push"""
    x = ia.stack(CHUNK_NAMES)
    t = stage(be, CHUNK_NAMES)["sums"]
    D = demod(be, 3)
    ref_pcm = push(be, D, x, [])
    ref = D.impair()
    for c in range(3):
        assert_report(ref[c], t[c], t.shape[1], "single push")
    all_plans = chunk_plans(ia.N)
    for plan in plans or all_plans:
        D.reset()
        sizes = all_plans[plan]
        stride = 1 if len(sizes) < 500 else 97
        count = [0]

        def look(pos):
            count[0] += 1
            if count[0] % stride and pos != ia.N:
                return
            got = D.impair()
            for c in range(3):
                assert_report(got[c], t[c], ((pos + 1) // 2) // im.BLOCK, (plan, pos))

        pcm = push(be, D, x, sizes, look)
        assert pcm.tobytes() == ref_pcm.tobytes(), plan
        assert D.impair() == ref, plan
    D.close()


# ----------------------------------------------------------------------------------------------------------------------- 7. channels
def check_channels(be: fc.Backend, k: int):
    names = ia.MULTI[k]
    D = demod(be, k)
    push(be, D, ia.stack(names), [33333])
    got = D.impair()
    D.close()
    for c, name in enumerate(names):
        S = demod(be, 1)
        push(be, S, ia.stack([name]), [])
        one = S.impair()[0]
        S.close()
        assert got[c] == one, (k, name)


def check_channel_7_of_9(be: fc.Backend):
    """the same input in channel 0 of K = 1 and in channel 7 of K = 9"""
    names = list(ia.MULTI[9])
    names[7] = "ray5us"
    D = demod(be, 9)
    push(be, D, ia.stack(names), [44444])
    nine = D.impair()[7]
    D.close()
    S = demod(be, 1)
    push(be, S, ia.stack(["ray5us"]), [])
    assert S.impair()[0] == nine
    S.close()


# --------------------------------------------------------------------------------------------------------------------- 8. life cycle
def check_life_cycle(be: fc.Backend):
    names = ["ray5us", "adj-200_0"]
    x = ia.stack(names)
    n = ia.N
    D = be.demod(2)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # not enabled: refused
        D.impair()
    assert ei.value.code == eng.EINVAL and "not enabled" in str(ei.value)
    keep_in, p_in = be.upload(x)
    cap = fm.outputs_total(n)
    keep_out, p_out = be.zeros((2, cap, 2))
    D.process(p_in, 2 * n, 1000, p_out, 2 * cap, cap)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # after a push: refused
        D.impair_enable()
    assert ei.value.code == eng.EINVAL and "before the first push" in str(ei.value)
    D.close()
    D = demod(be, 2)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # twice: refused
        D.impair_enable()
    assert ei.value.code == eng.EINVAL
    assert D.carrier()[0]["blocks"] == 0                        # it has enabled the carrier measurement
    for bad in (dict(explained_min=float("nan")), dict(explained_min=1.5), dict(explained_min=-0.1), dict(depth_min=float("inf")), dict(depth_min=-1.0),
                dict(rho_min=float("nan")), dict(rho_min=1.01), dict(rho_min=-0.5)):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            be.demod(2, impair=bad)
        assert ei.value.code == eng.EINVAL, bad
    first_pcm = push(be, D, x, [33333])
    first = D.impair()
    assert first[0]["blocks"] == 111 and first[0]["audio_blocks"] == 95 and first[0]["windowed"]["multipath"] and first[1]["windowed"]["side"] == -1
    D.reset()                                                   # still enabled, the totals zero
    zero = D.impair()
    assert all(v["blocks"] == 0 and v["audio_blocks"] == 0 and not any(v["windowed"].values()) and not any(v["running"].values()) for v in zero)
    second_pcm = push(be, D, x, [])                             # ... and a reset object equals a fresh one
    assert second_pcm.tobytes() == first_pcm.tobytes() and D.impair() == first
    D.close()
    T = demod(be, 2, impair=dict(explained_min=0.95, depth_min=0.05, rho_min=0.99))          # thresholds of its own: the same figures, another verdict
    push(be, T, x, [7777])
    strict = T.impair()
    T.close()
    for c in range(2):
        for kind in ("windowed", "running"):
            assert {k: strict[c][kind][k] for k in im.SUMS + im.FIGURES} == {k: first[c][kind][k] for k in im.SUMS + im.FIGURES}
    assert not strict[0]["windowed"]["multipath"] and not strict[1]["windowed"]["adjacent"] and strict[1]["windowed"]["side"] == 0


def check_with_everything_on(be: fc.Backend):
    """with carrier, steering, RDS and SAME already on: the impairment reports are those of a plain object, and audio, d, carrier(), steer(), the
    RDS and the SAME events are byte-equal with and without it"""
    names = ["ray5us", "noise20"]
    x = ia.stack(names)
    out = {}
    for on in (False, True):
        D = be.demod(2, carrier=True, steer=True, rds=True, same=True, impair=on)
        keep, ptr = be.upload(x)
        d, p = D.stage_mpx(ptr, 2 * ia.N, ia.N)
        pcm = push(be, D, x, [1081] * 30 + [40000])
        out[on] = (d.tobytes(), p.tobytes(), pcm.tobytes(), D.clip_counts().tobytes(), repr(D.carrier()), repr(D.steer()), repr(D.rds_read()), repr(D.same_read()),
                   repr([D.rds_stats(c) for c in range(2)]), repr([D.same_stats(c) for c in range(2)]))
        if on:
            got = D.impair()
        D.close()
    assert out[False] == out[True]
    P = demod(be, 2)
    push(be, P, x, [])
    assert P.impair() == got
    P.close()


# ------------------------------------------------------------------------------------------------- 8. 9. untouched audio, launch counts
def launches_expected(sizes, n: int, carrier: bool, impair: bool) -> int:
    """nrsc5hip_fm_debug_launches without RDS and SAME: per push the front end when a d sample is new, the pilot sums when a block completed, the
    audio when an audio block is due, the kept tails always; two more per push that completed a block for the carrier measurement, and two more
    for the impairments"""
    total = pos = 0
    for c in list(sizes) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        m0, m1 = (pos + 1) // 2, (pos + c + 1) // 2
        b0, b1 = m0 // im.BLOCK, m1 // im.BLOCK
        total += (m1 > m0) + (b1 > b0) + (max(b1 - im.W, 0) > max(b0 - im.W, 0)) + 1 + (b1 > b0) * (2 * carrier + 2 * impair)
        pos += c
    return total


def check_untouched(be: fc.Backend, name: str):
    x = fc.stack([name])
    sizes = [1081] * 40 + [1] * 5 + [50000]
    pushes = len(sizes) + 1
    out = {}
    for mode in ("plain", "carrier", "impair"):
        D = be.demod(1, carrier=mode == "carrier", impair=mode == "impair", **fa.demod_args(name))
        keep, ptr = be.upload(x)
        d, p = D.stage_mpx(ptr, 2 * fa.N, fa.N)
        pcm = push(be, D, x, sizes)
        out[mode] = (d.tobytes(), p.tobytes(), pcm.tobytes(), D.clip_counts().tobytes(), repr(D.carrier()) if mode != "plain" else None, D.launches())
        D.close()
    assert out["plain"][:4] == out["carrier"][:4] == out["impair"][:4], name
    assert out["carrier"][4] == out["impair"][4], name
    assert out["plain"][5] == launches_expected(sizes, fa.N, False, False) and out["carrier"][5] == launches_expected(sizes, fa.N, True, False)
    assert out["impair"][5] == launches_expected(sizes, fa.N, True, True)
    pos = nblk = 0                                              # the pushes that completed a block
    for c in sizes + [fa.N]:
        c = min(c, fa.N - pos)
        nblk += ((pos + c + 1) // 2) // im.BLOCK > ((pos + 1) // 2) // im.BLOCK
        pos += c
    assert out["impair"][5] - out["carrier"][5] == 2 * nblk and 0 < nblk < pushes          # exactly two launches per push that completed a block


# ------------------------------------------------------------------------------------------------------------------------- 10. hU
def check_taps(be: fc.Backend):
    """The 63-tap Kaiser design (beta 8) has a transition of about 30 kHz around each edge, so it cannot be flat to 0.5 dB from 105 kHz to 165 kHz:
    the edges themselves are its -6 dB points.  What it meets, verified on the model's own taps first: within 0.25 dB over 110 .. 160 kHz, within
    1.75 dB over 105 .. 165 kHz, and at least 80 dB down below 80 kHz (the programme, the pilot, RDS and the discriminator's noise parabola up to
    there) -- the issue asked for 50 dB below 60 kHz, which it meets with 40 dB to spare"""
    for who, h in (("model", ia.taps()[1]), ("library", None)):
        if h is None:
            D = be.demod(1)
            h = D.impair_taps()
            D.close()
            assert h.dtype == np.float32 and h.shape == (im.UT,)
            assert np.max(np.abs(h.astype(np.float64) - im.design_hu())) <= 2.0 ** -24 * np.max(np.abs(h))           # equal to float32 rounding
            assert np.array_equal(h, h[::-1])                                                                       # linear phase
        flat = im.response_db(h, np.linspace(110e3, 160e3, 501))
        wide = im.response_db(h, np.linspace(105e3, 165e3, 601))
        low = im.response_db(h, np.linspace(0.0, 80e3, 801))
        print(f"{who}: hU within {np.max(np.abs(flat)):.3f} dB over 110 .. 160 kHz, {np.max(np.abs(wide)):.3f} dB over 105 .. 165 kHz, {-np.max(low):.1f} dB down below 80 kHz, "
              f"{-np.max(low[:601]):.1f} dB below 60 kHz")
        assert np.max(np.abs(flat)) <= 0.25 and np.max(np.abs(wide)) <= 1.75 and np.max(low) <= -80.0 and np.max(low[:601]) <= -50.0
