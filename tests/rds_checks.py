"""The checks of RDS on the analog FM object (nrsc5hip_fm_rds_*, nrsc5_amd/csrc/k_rds.hip), written once and run twice: by
tests/test_rds_stage_cpu.py on the CPU-emulated twin and by tests/test_gpu_rds_stage.py on gfx950.  The reference is the float64 restatement
tests/rds_model.py on the inputs of tests/rds_args.py.

Bounds.  y through the stage hook: 4 x the largest |float32 model - float64 model| of the same input (the rule fm_checks uses for d); the window
energies: the same rule on the energies.  s_w, every bit, every event, the snapshot and the counters: exact -- rds_args asserts on every input
that no decision is within reach of those bounds.  The measured figures are in profiles/wideband_rds_cases.txt."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import fm_args as fa, fm_checks as fc, rds_args as ra, rds_model as rm


class Backend(fc.Backend):
    def demod(self, nchan: int, rds=True, **kw):
        return eng.FmDemod(nchan, lib_path=self.lib_path, rds=rds, **kw)


def stack(names) -> np.ndarray:
    return np.stack([ra.host(n) for n in names])


def event_key(e: dict):
    return (e["kind"], e["group"], e["bit"], tuple(e["v"]), bytes(e["data"]))


def model_events(g: rm.Groups) -> list:
    return [event_key(e) for e in g.events]


def split_events(events, nchan: int) -> list:
    out = [[] for _ in range(nchan)]
    last = -1
    for e in events:
        assert e["channel"] >= last                                            # channel by channel
        last = e["channel"]
        out[e["channel"]].append(event_key(e))
    return out


def session(be: Backend, D, x: np.ndarray, chunks):
    """push x (int16 [K, n, 2]) in the given chunk sizes (the last one takes the rest) -> (events per channel, snapshots, stats, pcm)"""
    k, n = x.shape[0], x.shape[1]
    keep_in, p_in = be.upload(x)
    cap = D.outputs_for(n) + 64
    keep_out, p_out = be.zeros((k, cap, 2))
    pos = got = 0
    for c in list(chunks) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        got += D.process(p_in + 4 * pos, 2 * n, c, p_out + 4 * got, 2 * cap, cap - got)
        pos += c
    assert pos == n
    events = split_events(D.rds_read(), k)
    assert D.rds_read() == []                                                  # delivered once
    return events, [D.rds_get(c) for c in range(k)], [D.rds_stats(c) for c in range(k)], be.download(keep_out)[:, :got].copy()


def compare_session(events, snap, stats, name: str):
    g = ra.reference(name)["groups"]
    assert events == model_events(g), (name, events, model_events(g))
    assert snap == g.snapshot(), (name, snap, g.snapshot())
    assert stats == g.stats, (name, {k: (stats[k], g.stats[k]) for k in stats if stats[k] != g.stats[k]})


# ------------------------------------------------------------------------------------------------------------------------ tables
def check_tables(be: Backend):
    D = be.demod(1)
    tab = D.rds_tables()
    want = rm.design_taps()
    assert tab.shape == (rm.GRID, rm.NT) == (D.rds_phases, D.rds_taps) and D.rds_points_per_bit == rm.S and D.rds_window_bits == rm.WIN_BITS
    assert D.rds_latency_in == rm.LATENCY_IN == 96431
    assert np.max(np.abs(tab.astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want))             # equal to float32 rounding
    assert np.array_equal(tab, ra.tables()[1])
    # the window reaches 2 T either way and no further, and the symbol is odd about the grid point (a biphase symbol centred on it)
    assert tab[0, 0] == 0.0 and tab[0, -1] == 0.0 and np.all(tab[:, 0] == 0.0)
    assert np.max(np.abs(want[0] + want[0][::-1])) < 1e-12
    # its spectrum is the biphase symbol's, cos(pi f T / 4) sin(pi f T / 2): a null at DC, the peak where that product has it (931 Hz), nothing
    # beyond 2 / T = 2375 Hz but the window's skirt
    H = np.abs(np.fft.rfft(want[0], 1 << 18))
    fr = np.arange(H.size) * fm_fs1() / (1 << 18)
    xs = np.linspace(0.0, 2.0, 20001)
    peak = xs[np.argmax(np.cos(np.pi * xs / 4) * np.sin(np.pi * xs / 2))] * 1187.5
    assert H[0] < 1e-9 * H.max() and abs(fr[np.argmax(H)] - peak) < 30.0, (fr[np.argmax(H)], peak)
    assert np.max(H[fr > 3200.0]) < 1e-3 * H.max(), np.max(H[fr > 3200.0]) / H.max()
    D.close()


def fm_fs1() -> float:
    from tests import fm_model as fm
    return fm.FS1


# ------------------------------------------------------------------------------------------------ signal level through the stage hook
def check_stage_signal(be: Backend, names=None) -> list:
    """-> the lines of profiles/wideband_rds_cases.txt"""
    names = list(names or ra.CASES)
    D = be.demod(len(names))
    keep, ptr = be.upload(stack(names))
    got = D.stage_rds_mf(ptr, 2 * ra.N, ra.N)
    assert D.rds_read() == [] and D.rds_stats(0)["bits"] == 0                   # the object's own session is untouched
    D.close()
    lines = []
    for c, name in enumerate(names):
        ref = ra.reference(name)
        assert got["y"][c].shape == ref["y"].shape and got["energy"][c].shape == ref["energy"].shape
        err_y = float(np.max(np.abs(got["y"][c].astype(np.complex128) - ref["y"])))
        err_e = float(np.max(np.abs(got["energy"][c].astype(np.float64) - ref["energy"])))
        line = (f"{name:8s} y within {err_y:.3g} (bound {ref['tol_y']:.3g}), energies within {err_e:.3g} (bound {ref['tol_e']:.3g}), s {[int(v) for v in got['s'][c]]}, "
                f"smallest margin: bits {ref['margin_bit']:.3g} x, energies {ref['margin_e']:.3g} x the bound")
        print(line)
        lines.append(line)
        assert err_y <= ref["tol_y"], (name, err_y, ref["tol_y"])
        assert err_e <= ref["tol_e"], (name, err_e, ref["tol_e"])
        assert np.array_equal(got["s"][c], ref["s"]), (name, got["s"][c], ref["s"])
        assert len(got["bits"][c]) == len(ref["bits"])
        for w, (a, b) in enumerate(zip(got["bits"][c], ref["bits"])):
            assert np.array_equal(a, b), (name, w, int(np.sum(a != b)) if a.size == b.size else (a.size, b.size))
    return lines


# -------------------------------------------------------------------------------------------------------------- whole sessions
def check_session_case(be: Backend, name: str):
    D = be.demod(1)
    events, snap, stats, _ = session(be, D, stack([name]), [])
    D.close()
    compare_session(events[0], snap[0], stats[0], name)


def check_multi(be: Backend, k: int):
    names = ra.MULTI[k]
    D = be.demod(k)
    events, snap, stats, _ = session(be, D, stack(names), [200001])
    D.close()
    for c, name in enumerate(names):
        compare_session(events[c], snap[c], stats[c], name)


def chunk_plans(n: int):
    rng = np.random.default_rng(1187)
    return {"sevens": [7] * (n // 7 + 1), "1079": [1079] * (n // 1079 + 1), "1080": [1080] * (n // 1080 + 1), "1081": [1081] * (n // 1081 + 1),
            "random": list(rng.integers(1, 20000, 200)), "ones": [1] * 3000}


CHUNK_NAMES = ["wrap70", "nords", "wrap07"]


def check_chunking(be: Backend, plans=None):
    """three channels, one of them without RDS: every chunking gives the events, snapshot and counters of the single push, and the same audio"""
    x = stack(CHUNK_NAMES)
    D = be.demod(3)
    ref = session(be, D, x, [])
    for c, name in enumerate(CHUNK_NAMES):
        compare_session(ref[0][c], ref[1][c], ref[2][c], name)
    assert ref[0][0] and ref[0][2] and not ref[0][1]
    all_plans = chunk_plans(ra.N)
    for plan in plans or all_plans:
        D.reset()
        out = session(be, D, x, all_plans[plan])
        assert out[0] == ref[0] and out[1] == ref[1] and out[2] == ref[2], plan
        assert out[3].tobytes() == ref[3].tobytes(), plan
    D.close()


def check_reset_and_enable(be: Backend):
    x = stack(["stereo", "mono"])
    D = be.demod(2)
    first = session(be, D, x, [123457])
    D.reset()
    assert D.rds_read() == [] and D.rds_stats(0) == dict.fromkeys(eng.RDS_STATS, 0)
    s0 = D.rds_get(0)
    assert s0["pi"] == -1 and s0["ps"] is None and s0["rt"] is None and s0["clock"] is None and not s0["synced"]
    second = session(be, D, x, [])
    assert first[:3] == second[:3] and first[3].tobytes() == second[3].tobytes()       # a reset object equals a fresh one
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.rds_enable()                                                                   # twice
    assert ei.value.code == eng.EINVAL
    for bad in (-1, 2):
        with pytest.raises(eng.Nrsc5HipError):
            D.rds_get(bad)
        with pytest.raises(eng.Nrsc5HipError):
            D.rds_stats(bad)
    D.close()
    # enabling after the first push is rejected, and the calls of an object without RDS say so
    D = be.demod(1, rds=False)
    for call in (D.rds_read, lambda: D.rds_get(0), lambda: D.rds_stats(0)):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            call()
        assert ei.value.code == eng.EINVAL and "not enabled" in str(ei.value)
    keep_in, p_in = be.upload(stack(["stereo"])[:, :1000])
    keep_out, p_out = be.zeros((1, 64, 2))
    D.process(p_in, 2000, 1000, p_out, 128, 64)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.rds_enable()
    assert ei.value.code == eng.EINVAL and "before the first push" in str(ei.value)
    D.reset()
    with pytest.raises(eng.Nrsc5HipError):
        D.rds_enable()                                                                   # a reset does not reopen it
    D.close()
    for burst in (-1, 3):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            be.demod(1, rds_correct_burst=burst)
        assert ei.value.code == eng.EINVAL


def check_audio_untouched(be: Backend):
    """an existing fm_args case: the object without RDS and the object with it deliver the same audio bytes and clip counts, and both are the
    float64 audio model's within fm_checks' bound"""
    names = ["lr80", "cnr40", "l1k"]
    x = fc.stack(names)
    off = be.demod(3, rds=False)
    pcm0, clips0 = fc.run(be, off, x, [50000])
    off.close()
    on = be.demod(3, rds=True)
    pcm1, clips1 = fc.run(be, on, x, [50000])
    assert on.rds_read() == [] and on.rds_stats(0)["bits"] == 151               # one window of a host without RDS: bits, no event
    on.close()
    assert pcm0.tobytes() == pcm1.tobytes() and np.array_equal(clips0, clips1)
    for c, name in enumerate(names):
        fc.compare(pcm0[c], clips0[c], name)


def expected_launches(n: int, chunks, rds: bool):
    """kernel launches of a session from the definitions alone -> (audio path, RDS): per push the front end when a d sample is new, the pilot sums
    when a block is complete, the audio when an audio block is due, the kept tails always; with RDS the matched filter when a grid point is new
    and, when a window was decided, decisions, groups and the kept y"""
    from tests import fm_model as fm
    audio = extra = 0
    pos = m0 = b0 = a0 = r0 = w0 = 0
    for c in list(chunks) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        pos += c
        m1 = (pos + 1) // 2
        b1 = m1 // fm.BLOCK
        a1 = max(0, b1 - fm.W)
        audio += (m1 > m0) + (b1 > b0) + (a1 > a0) + 1
        if rds:
            r1 = rm.points_total(m1)
            w1 = r1 // rm.WIN_PTS
            extra += (r1 > r0) + 3 * (w1 > w0)
            r0, w0 = r1, w1
        m0, b0, a0 = m1, b1, a1
    return audio, extra


def check_launch_counts(be: Backend):
    """an fm_args case: the object without RDS launches what it did before RDS existed -- front, pilot sums, audio, kept tails: 4 for a session in
    one push -- and the object with RDS that plus its own launches"""
    names = ["lr80", "cnr40", "l1k"]
    x = fc.stack(names)
    plans = {"one": [], "two": [50000], "ones": [1] * 3000, "1080": [1080] * (fa.N // 1080 + 1)}
    off, on = be.demod(3, rds=False), be.demod(3, rds=True)
    assert off.launches() == 0 and on.launches() == 0
    for plan, chunks in plans.items():
        off.reset(); on.reset()
        fc.run(be, off, x, chunks)
        fc.run(be, on, x, chunks)
        audio, extra = expected_launches(fa.N, chunks, True)
        assert expected_launches(fa.N, chunks, False) == (audio, 0)
        print(f"{plan}: launches without RDS {off.launches()} (expected {audio}), with RDS {on.launches()} (expected {audio} + {extra})")
        assert off.launches() == audio, (plan, off.launches(), audio)
        assert on.launches() == audio + extra, (plan, on.launches(), audio, extra)
        if plan == "one":
            assert (audio, extra) == (4, 4)              # front + pilot + audio + keep; matched filter + decisions + groups + kept y (one window)
        if plan == "two":
            assert (audio, extra) == (8, 5)              # grid points are new in both pushes, the one window is decided in the second
    keep, ptr = be.upload(x)
    before = on.launches()
    on.stage_rds_mf(ptr, 2 * fa.N, fa.N)
    on.stage_mpx(ptr, 2 * fa.N, fa.N)
    assert on.launches() == before                         # the stage hooks run sessions of their own
    on.reset()
    assert on.launches() == 0
    off.close(); on.close()


# ------------------------------------------------------------------------------------------------------------------ group level
def run_groups(be: Backend, name: str, pieces=None):
    bits, rst, raw, burst = ra.group_cases()[name]
    D = be.demod(2, rds_raw_groups=raw, rds_correct_burst=burst)
    events = []
    if pieces is None:
        D.stage_rds_groups([bits], channels=[1], reset_at=None if rst is None else [rst])
        events += D.rds_read()
    else:                                                                      # the stream ends mid-block and continues in the next call
        assert rst is None
        for a, b in zip([0] + pieces, pieces + [bits.size]):
            D.stage_rds_groups([bits[a:b]], channels=[1])
            events += D.rds_read()
    snap, stats, other = D.rds_get(1), D.rds_stats(1), D.rds_stats(0)
    D.close()
    assert other == dict.fromkeys(eng.RDS_STATS, 0)                            # the channel not listed is untouched
    g = ra.group_reference(name)
    got = split_events(events, 2) if pieces is None else [[], [event_key(e) for e in events]]
    want = model_events(g)
    if rst is not None:                                                        # what was reported in front of the reset comes first
        head = rm.Groups(burst, raw).push(bits[:rst])
        want = model_events(head) + want
    assert got[0] == [] and got[1] == want, (name, len(got[1]), len(want))
    assert snap == g.snapshot(), (name, snap, g.snapshot())
    assert stats == g.stats, (name, {k: (stats[k], g.stats[k]) for k in stats if stats[k] != g.stats[k]})


def check_groups_case(be: Backend, name: str):
    run_groups(be, name)


def check_groups_in_pieces(be: Backend):
    n = ra.group_cases()["schedule"][0].size
    run_groups(be, "schedule", pieces=[1000 + 13, 1000 + 13 + 1, 5000 + 7])
    run_groups(be, "deleted_bit", pieces=[104 * 5 + 41])
    assert n > 5007


def check_groups_many_channels(be: Backend):
    """several channels in one call, listed out of order, one of them empty"""
    names = ["schedule", "single_bit_errors", "noise_in_front"]
    D = be.demod(5)
    D.stage_rds_groups([ra.group_cases()[n][0] for n in names] + [np.zeros(0, np.uint8)], channels=[4, 0, 2, 3])
    events = split_events(D.rds_read(), 5)
    for ch, name in zip([4, 0, 2], names):
        g = ra.group_reference(name)
        assert events[ch] == model_events(g) and D.rds_get(ch) == g.snapshot() and D.rds_stats(ch) == g.stats, name
    assert events[1] == [] and events[3] == [] and D.rds_stats(3)["bits"] == 0
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_rds_groups([np.zeros(4, np.uint8)] * 2, channels=[1, 1])          # a channel listed twice
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_rds_groups([np.zeros(4, np.uint8)], channels=[5])
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_rds_groups([np.zeros(4, np.uint8)], reset_at=[5])
    D.close()
