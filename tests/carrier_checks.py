"""The checks of the carrier measurement (nrsc5hip_fm_carrier*, nrsc5_amd/csrc/k_fm_carrier.hip), written once and run twice: by
tests/test_carrier_stage_cpu.py on the CPU-emulated twin and by tests/test_gpu_carrier_stage.py on gfx950.  The reference is the float64
restatement tests/carrier_model.py on the inputs of tests/carrier_args.py.

Bounds.  r and the block triples through the stage hook: 4 x the largest |float32 model - float64 model| of the same input and quantity (the
project's rule for d).  The sums with a stated order -- the windowed and the running triple -- are compared bit for bit with the model's sums of
the device's own block triples, and the figures with the formula applied to those sums (1e-9 dB / Hz: two libm's log10).  Physical bounds: the
issue's (0.5 dB, 50 Hz, 0.1 dB), taken on the windowed report of the last audio block -- 33 blocks behind the start of the stream, where the
channel filter's turn-on (x[n] = 0 for n < 0: 28 samples without a carrier) no longer weighs; that transient alone holds the running cnr_db of
a 111-block session under 36 dB."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import carrier_args as ca, carrier_model as cm, fm_args as fa, fm_checks as fc, fm_model as fm

FIG_TOL = 1e-9


def demod(be: fc.Backend, nchan: int, carrier: bool = True, **kw):
    return be.demod(nchan, carrier=carrier, **kw)


def push(be: fc.Backend, D, x: np.ndarray, chunks, each=None):
    """push x (int16 [K, n, 2]) in the given chunk sizes (the last takes the rest) -> pcm [K, frames, 2]; each(pos) is called after every push"""
    k, n = x.shape[0], x.shape[1]
    keep_in, p_in = be.upload(x)
    cap = fm.outputs_total(n) + 64
    keep_out, p_out = be.zeros((k, cap, 2))
    pos = got = 0
    for c in list(chunks) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        got += D.process(p_in + 4 * pos, 2 * n, c, p_out + 4 * got, 2 * cap, cap - got)
        pos += c
        if each:
            each(pos)
    assert pos == n and got == fm.outputs_total(n)
    return be.download(keep_out)[:, :got].copy()


def stage(be: fc.Backend, names):
    D = be.demod(len(names))                                   # the hook needs no enabled object
    keep, ptr = be.upload(ca.stack(names))
    r, t = D.stage_carrier(ptr, 2 * ca.N, ca.N)
    D.close()
    return r, t


def assert_report(got: dict, t: np.ndarray, blocks: int, what=""):
    """one channel's nrsc5hip_fm_carrier against the model's sums of the block triples t, bit for bit, and the figures by the formula"""
    want = cm.reports(t[:blocks])
    assert got["blocks"] == want["blocks"] and got["audio_blocks"] == want["audio_blocks"], (what, got, want)
    for kind in ("windowed", "running"):
        for q in ("sum2", "sum4", "sum1", "count"):
            assert got[kind][q] == want[kind][q], (what, kind, q, got[kind][q], want[kind][q])
        for q in ("level_db", "cnr_db", "offset_hz"):
            assert np.isfinite(got[kind][q]), (what, kind, q)
            assert abs(got[kind][q] - want[kind][q]) <= FIG_TOL * max(1.0, abs(want[kind][q])), (what, kind, q, got[kind][q], want[kind][q])


# ------------------------------------------------------------------------------------------------- 1. sums against the model (stage hook)
def check_stage_sums(be: fc.Backend, names=None):
    names = list(names or ca.CASES)
    r, t = stage(be, names)
    assert r.shape == (len(names), ca.N // 2) and t.shape == (len(names), ca.N // 2 // cm.BLOCK, 3)
    for c, name in enumerate(names):
        ref = ca.reference(name)
        err_r = float(np.max(np.abs(r[c].astype(np.float64) - ref["r"])))
        err_t = np.max(np.abs(t[c] - ref["t"]), axis=0)
        print(f"{name}: r within {err_r:.3g} of the float64 model (bound {4 * ref['r_err32']:.3g}, r up to {ref['r'].max():.3g}); block sums within "
              f"{err_t[0]:.3g} / {err_t[1]:.3g} / {err_t[2]:.3g} (bounds {4 * ref['t_err32'][0]:.3g} / {4 * ref['t_err32'][1]:.3g} / {4 * ref['t_err32'][2]:.3g})")
        assert np.all(np.isfinite(r[c])) and np.all(np.isfinite(t[c]))
        assert err_r <= 4 * ref["r_err32"], (name, err_r, 4 * ref["r_err32"])
        assert np.all(err_t <= 4 * ref["t_err32"]), (name, err_t, 4 * ref["t_err32"])
    return r, t


# ---------------------------------------------------------------------------------------------------------------------- 2. the report
def check_report(be: fc.Backend):
    names = list(ca.CASES)
    r, t = stage(be, names)
    d = stage_d(be, names)
    for c in range(len(names)):                               # the block triples are the stated sums of the device's own r and d, bit for bit
        assert np.array_equal(cm.block_sums_in_order(r[c], d[c]), t[c]), names[c]
    D = demod(be, len(names))
    assert all(v["blocks"] == 0 and v["running"]["count"] == 0 and not any(v["windowed"].values()) and not any(v["running"].values()) for v in D.carrier())
    push(be, D, ca.stack(names), [50000])
    got = D.carrier()
    D.close()
    for c, name in enumerate(names):
        assert_report(got[c], t[c], t.shape[1], name)
        print(f"{name}: windowed level {got[c]['windowed']['level_db']:.2f} dBFS cnr {got[c]['windowed']['cnr_db']:.2f} dB offset {got[c]['windowed']['offset_hz']:.1f} Hz; "
              f"running cnr {got[c]['running']['cnr_db']:.2f} dB")
    by = dict(zip(names, got))
    for kind in ("windowed", "running"):
        z = by["zero"][kind]
        assert z["level_db"] == cm.DB_MIN and z["cnr_db"] == cm.DB_MIN and z["offset_hz"] == 0.0          # the clamps: no power at all
        n = by["noise"][kind]
        assert n["cnr_db"] == cm.DB_MIN or n["cnr_db"] < 0.0, n                                          # no carrier
        s = by["silent"][kind]
        assert np.isfinite(s["cnr_db"]) and cm.DB_MIN < s["cnr_db"] <= cm.DB_MAX and s["cnr_db"] > 30.0, s   # a clean carrier: finite
    assert np.isfinite(by["silent"]["windowed"]["cnr_db"]) and by["silent"]["windowed"]["cnr_db"] > 60.0


def stage_d(be: fc.Backend, names) -> np.ndarray:
    D = be.demod(len(names))
    keep, ptr = be.upload(ca.stack(names))
    d, _ = D.stage_mpx(ptr, 2 * ca.N, ca.N)
    D.close()
    return d


# ------------------------------------------------------------------------------------------------------------ 3. physical condition
def physical(rep: dict, name: str, who: str):
    amp = ca.CASES[name][1]
    w = rep["windowed"]
    line = f"{who} {name}: level {w['level_db']:.3f} dBFS (carrier {20 * np.log10(amp / 32768):.3f}), cnr {w['cnr_db']:.2f} dB, offset {w['offset_hz']:.1f} Hz"
    if name in ca.CNR_CASES:
        want = ca.CNR_CASES[name] + cm.FILTER_GAIN_DB
        line += f" (in-filter CNR {want:.2f} dB)"
        print(line)
        assert abs(w["cnr_db"] - want) <= 0.5, (who, name, w["cnr_db"], want)
    else:
        print(line)
        assert abs(w["offset_hz"] - ca.SHIFT_CASES[name]) <= 50.0, (who, name, w["offset_hz"])
        assert abs(rep["running"]["offset_hz"] - ca.SHIFT_CASES[name]) <= 50.0, (who, name, rep["running"]["offset_hz"])
    assert abs(w["level_db"] - 20 * np.log10(amp / 32768)) <= 0.1, (who, name, w["level_db"])


def check_physical(be: fc.Backend):
    assert abs(-ca.ha_noise_gain_db() - cm.FILTER_GAIN_DB) < 0.005, ca.ha_noise_gain_db()
    names = list(ca.CNR_CASES) + list(ca.SHIFT_CASES)
    for name in names:                                          # the definition first: a wrong one fails here, on the CPU
        physical(ca.reference(name)["reports"], name, "model")
    D = demod(be, len(names))
    push(be, D, ca.stack(names), [])
    got = D.carrier()
    D.close()
    for c, name in enumerate(names):
        physical(got[c], name, "library")


# ----------------------------------------------------------------------------------------------------------------------- 4. chunking
CHUNK_NAMES, CHUNK_GAINS = ["stereo25", "shift+1k5", "fullscale"], [1.0, 1.0, 4.0]


def check_chunking(be: fc.Backend, plans=None):
    """three channels, the last one clipping: after every look the reports equal the model's sums of the whole session's block triples up to
    the blocks complete by then, so every chunking gives the bits of the single push"""
    x = ca.stack(CHUNK_NAMES)
    _, t = stage(be, CHUNK_NAMES)
    D = demod(be, 3, gains=CHUNK_GAINS)
    ref_pcm = push(be, D, x, [])
    ref = D.carrier()
    assert D.clip_counts()[2].sum() > 0
    for c in range(3):
        assert_report(ref[c], t[c], t.shape[1], "single push")
    all_plans = fc.chunk_plans(ca.N)
    for plan in plans or all_plans:
        D.reset()
        sizes = all_plans[plan]
        stride = 1 if len(sizes) < 500 else 97
        count = [0]

        def look(pos):
            count[0] += 1
            if count[0] % stride and pos != ca.N:
                return
            got = D.carrier()
            for c in range(3):
                assert_report(got[c], t[c], ((pos + 1) // 2) // cm.BLOCK, (plan, pos))

        pcm = push(be, D, x, sizes, look)
        assert pcm.tobytes() == ref_pcm.tobytes(), plan
        assert D.carrier() == ref, plan
    D.close()


# ----------------------------------------------------------------------------------------------------------------------- 5. channels
def check_channels(be: fc.Backend, k: int):
    names = ca.MULTI[k]
    D = demod(be, k)
    push(be, D, ca.stack(names), [33333])
    got = D.carrier()
    D.close()
    for c, name in enumerate(names):
        S = demod(be, 1)
        push(be, S, ca.stack([name]), [])
        one = S.carrier()[0]
        S.close()
        assert got[c] == one, (k, name)


# --------------------------------------------------------------------------------------------------------------------- 6. life cycle
def check_life_cycle(be: fc.Backend):
    names = ["stereo25", "silent15"]
    x = ca.stack(names)
    n = ca.N
    D = be.demod(2)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # not enabled: refused
        D.carrier()
    assert ei.value.code == eng.EINVAL and "not enabled" in str(ei.value)
    keep_in, p_in = be.upload(x)
    cap = fm.outputs_total(n)
    keep_out, p_out = be.zeros((2, cap, 2))
    D.process(p_in, 2 * n, 1000, p_out, 2 * cap, cap)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # after a push: refused
        D.carrier_enable()
    assert ei.value.code == eng.EINVAL and "before the first push" in str(ei.value)
    D.close()
    D = demod(be, 2)
    with pytest.raises(eng.Nrsc5HipError) as ei:                # twice: refused
        D.carrier_enable()
    assert ei.value.code == eng.EINVAL
    first_pcm = push(be, D, x, [33333])
    first = D.carrier()
    assert first[0]["blocks"] == 111 and first[0]["audio_blocks"] == 95 and first[0]["running"]["cnr_db"] > 20.0
    D.reset()                                                   # still enabled, the totals zero
    zero = D.carrier()
    assert all(v["blocks"] == 0 and v["audio_blocks"] == 0 and not any(v["windowed"].values()) and not any(v["running"].values()) for v in zero)
    D.process(p_in, 2 * n, 40000, p_out, 2 * cap, cap)
    before = D.carrier()
    assert before[0]["blocks"] == 37 and before[0]["audio_blocks"] == 21
    with pytest.raises(eng.Nrsc5HipError) as ei:                # EOVERFLOW leaves the totals untouched
        D.process(p_in + 4 * 40000, 2 * n, n - 40000, p_out, 2 * cap, 10)
    assert ei.value.code == eng.EOVERFLOW
    assert D.carrier() == before
    D.reset()
    second_pcm = push(be, D, x, [])                             # ... and a reset object equals a fresh one
    assert second_pcm.tobytes() == first_pcm.tobytes() and D.carrier() == first
    D.close()
    F = demod(be, 2)
    push(be, F, x, [7777])
    assert F.carrier() == first
    F.close()


# ----------------------------------------------------------------------------------------------------------------- 7. untouched audio
def launches_expected(sizes, n: int) -> int:
    """what nrsc5hip_fm_debug_launches states per push without RDS and without the measurement: the front end when a d sample is new, the pilot
    sums when a block completed, the audio when an audio block is due, the kept tails always"""
    total = pos = 0
    for c in list(sizes) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        m0, m1 = (pos + 1) // 2, (pos + c + 1) // 2
        b0, b1 = m0 // cm.BLOCK, m1 // cm.BLOCK
        total += (m1 > m0) + (b1 > b0) + (max(b1 - cm.W, 0) > max(b0 - cm.W, 0)) + 1
        pos += c
    return total


def check_untouched_audio(be: fc.Backend, name: str):
    x = fc.stack([name])
    sizes = [1081] * 40 + [1] * 5 + [50000]
    out = {}
    for on in (False, True):
        D = demod(be, 1, carrier=on, **fa.demod_args(name))
        keep, ptr = be.upload(x)
        d, p = D.stage_mpx(ptr, 2 * fa.N, fa.N)
        pcm = push(be, D, x, sizes)
        out[on] = (d.tobytes(), p.tobytes(), pcm.tobytes(), D.clip_counts().tobytes(), D.launches())
        D.close()
    assert out[False][:4] == out[True][:4], name
    assert out[False][4] == launches_expected(sizes, fa.N), (out[False][4], launches_expected(sizes, fa.N))
    assert out[True][4] > out[False][4]                         # the measurement's own launches are counted
    want = fa.reference(name)[0]
    got = np.frombuffer(out[True][2], dtype=np.int16).reshape(-1, 2)
    assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1
