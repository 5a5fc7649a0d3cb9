"""The checks of SAME on the analog FM object (nrsc5hip_fm_same_*, nrsc5_amd/csrc/k_same.hip), written once and run twice: by
tests/test_same_stage_cpu.py on the CPU-emulated twin and by tests/test_gpu_same_stage.py on gfx950.  The reference is the float64 restatement
tests/same_model.py on the inputs of tests/same_args.py.

Bounds.  c, q and the metrics through the stage hook: 4 x the largest |float32 model - float64 model| of the same input, computed in
same_args.analyse (the rule fm_checks uses for d).  s_w: exact -- same_args asserts on every input that no window's choice is within reach of
float32 rounding.  Bits: exact wherever the model's |q| exceeds the bound of q; the others are counted and printed, and same_args asserts that
none lies inside a burst.  Events, snapshot and counters: exact."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import fm_args as fa, fm_checks as fc, rds_checks as rc, same_args as sa, same_model as sm


class Backend(fc.Backend):
    def demod(self, nchan: int, same=True, **kw):
        return eng.FmDemod(nchan, lib_path=self.lib_path, same=same, **kw)


def stack(names, n: int = sa.N) -> np.ndarray:
    return np.stack([sa.host(k)[:n] for k in names])


def event_key(e: dict):
    return (e["kind"], e["first"], e["last"], tuple(e["v"]), bytes(e["data"]))


def model_events(g: sm.Framer) -> list:
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
    events = split_events(D.same_read(), k)
    assert D.same_read() == []                                                 # delivered once
    return events, [D.same_get(c) for c in range(k)], [D.same_stats(c) for c in range(k)], be.download(keep_out)[:, :got].copy()


def compare_session(events, snap, stats, ref: dict, what):
    g = ref["framer"]
    assert events == model_events(g), (what, events, model_events(g))
    assert snap == g.snapshot(), (what, snap, g.snapshot())
    assert stats == g.stats, (what, {k: (stats[k], g.stats[k]) for k in stats if stats[k] != g.stats[k]})


# ------------------------------------------------------------------------------------------------------------------------ the table
def check_table(be: Backend):
    D = be.demod(1)
    tab = D.same_table()
    want = sm.table()
    assert tab.shape == (sm.DEN, 2) and D.same_points_per_bit == sm.S and D.same_window_bits == sm.WIN_BITS
    assert D.same_latency_in == sm.LATENCY_IN == 92693
    assert np.max(np.abs(tab.astype(np.float64) - want)) <= 2.0 ** -24                                    # equal to float32 rounding
    assert np.array_equal(tab, sa.tables()[1])
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0
    # the grid: 8 points per bit, 50 bits are 35721 samples exactly, segments of 89 or 90 samples; both tones close on a bit
    g = sm.grid(np.arange(401, dtype=np.int64))
    assert g[400] == sm.DEN and set(np.diff(g).tolist()) == {89, 90}
    assert (sm.K_MARK, sm.K_SPACE) == (4 * 50, 3 * 50)                                                    # four and three cycles per bit of DEN / 50 samples
    # a window is decided exactly from the latency on: one sample less and the stage hook sees no window
    keep, ptr = be.upload(stack(["eom"], sm.LATENCY_IN))
    assert D.stage_same_tones(ptr, 2 * sm.LATENCY_IN, sm.LATENCY_IN)["s"].shape == (1, 1)
    assert D.stage_same_tones(ptr, 2 * sm.LATENCY_IN, sm.LATENCY_IN - 1)["s"].shape == (1, 0)
    D.close()


# ------------------------------------------------------------------------------------------------ signal level through the stage hook
def check_stage_signal(be: Backend, names=None) -> list:
    """-> one line per input: what was measured against its bounds"""
    names = list(names or sa.CASES)
    D = be.demod(len(names))
    keep, ptr = be.upload(stack(names))
    got = D.stage_same_tones(ptr, 2 * sa.N, sa.N)
    assert D.same_read() == [] and D.same_stats(0)["bits"] == 0                 # the object's own session is untouched
    D.close()
    lines = []
    for c, name in enumerate(names):
        ref = sa.reference(name)
        nq = ref["s"].size * sm.WIN_PTS
        assert got["c"][c].shape == ref["c"].shape and got["q"][c].shape == (nq,) and got["metric"][c].shape == ref["metric"].shape
        err_c = float(np.max(np.abs(got["c"][c].astype(np.complex128) - ref["c"])))
        err_q = float(np.max(np.abs(got["q"][c].astype(np.float64) - ref["q"][:nq])))
        err_m = float(np.max(np.abs(got["metric"][c].astype(np.float64) - ref["metric"])))
        weak = differ_weak = 0
        assert len(got["bits"][c]) == len(ref["bits"])
        line = (f"{name:9s} c within {err_c:.3g} (bound {ref['tol_c']:.3g}), q within {err_q:.3g} (bound {ref['tol_q']:.3g}), metrics within {err_m:.3g} "
                f"(bound {ref['tol_m']:.3g}), s {[int(v) for v in got['s'][c]]}, smallest timing margin {ref['margin_m']:.3g} x its bound")
        print(line)
        assert err_c <= ref["tol_c"], (name, err_c, ref["tol_c"])
        assert err_q <= ref["tol_q"], (name, err_q, ref["tol_q"])
        assert err_m <= ref["tol_m"], (name, err_m, ref["tol_m"])
        assert np.array_equal(got["s"][c], ref["s"]), (name, got["s"][c], ref["s"])
        for w, (a, b, wk) in enumerate(zip(got["bits"][c], ref["bits"], ref["weak"])):
            assert a.size == b.size, (name, w, a.size, b.size)
            assert np.array_equal(a[~wk], b[~wk]), (name, w, int(np.sum(a[~wk] != b[~wk])))
            weak += int(wk.sum())
            differ_weak += int(np.sum(a[wk] != b[wk]))
        line += f", bits within the bound of q: {weak} ({differ_weak} of them differ)"
        print(f"{name}: {weak} bits within the bound of q, {differ_weak} of them differ")
        lines.append(line)
        if name == "zero":
            assert not got["c"][c].any() and not any(b.any() for b in got["bits"][c])                      # d = 0 throughout: all-zero bits
    return lines


# -------------------------------------------------------------------------------------------------------------- whole sessions
def check_session_case(be: Backend, name: str):
    D = be.demod(1)
    events, snap, stats, _ = session(be, D, stack([name]), [])
    D.close()
    compare_session(events[0], snap[0], stats[0], sa.reference(name), name)


def check_multi(be: Backend, k: int):
    names = sa.MULTI[k]
    D = be.demod(k)
    events, snap, stats, _ = session(be, D, stack(names), [200001])
    D.close()
    for c, name in enumerate(names):
        compare_session(events[c], snap[c], stats[c], sa.reference(name), name)


CHUNK_NAMES = ["eom", "programme", "seam"]


def chunk_plans(n: int = sa.N_SHORT) -> dict:
    """RDS's plans, on the short session; its pushes of 7 samples are taken across the decision of the first window (2000 of them from 7000
    samples in front of it, the rest in one push) -- a session in sevens alone is 50 000 pushes and two minutes on the twin"""
    plans = rc.chunk_plans(n)
    plans["sevens"] = [sm.LATENCY_IN - 7 * 1000 + 3] + [7] * 2000
    return plans


def check_chunking(be: Backend, plans=None):
    """three channels, one of them without a burst: every chunking gives the events, snapshot and counters of the single push, and the same audio"""
    x = stack(CHUNK_NAMES, sa.N_SHORT)
    D = be.demod(3)
    ref = session(be, D, x, [])
    for c, name in enumerate(CHUNK_NAMES):
        compare_session(ref[0][c], ref[1][c], ref[2][c], sa.reference_short(name), name)
    assert ref[0][0] and ref[0][2] and not ref[0][1]
    all_plans = chunk_plans()
    for plan in plans or all_plans:
        D.reset()
        out = session(be, D, x, all_plans[plan])
        assert out[0] == ref[0] and out[1] == ref[1] and out[2] == ref[2], plan
        assert out[3].tobytes() == ref[3].tobytes(), plan
    D.close()


def check_reset_and_enable(be: Backend):
    x = stack(["eom", "header"])
    D = be.demod(2)
    first = session(be, D, x, [123457])
    D.reset()
    assert D.same_read() == [] and D.same_stats(0) == dict.fromkeys(eng.SAME_STATS, 0)
    s0 = D.same_get(0)
    assert s0 == {"text": None, "kind": None, "first": -1, "last": -1, "group_bursts": 0, "group_kind": None, "in_message": 0}
    second = session(be, D, x, [])
    assert first[:3] == second[:3] and first[3].tobytes() == second[3].tobytes()       # a reset object equals a fresh one
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.same_enable()                                                                  # twice
    assert ei.value.code == eng.EINVAL
    for bad in (-1, 2):
        with pytest.raises(eng.Nrsc5HipError):
            D.same_get(bad)
        with pytest.raises(eng.Nrsc5HipError):
            D.same_stats(bad)
    D.close()
    # enabling after the first push is rejected, and the calls of an object without SAME say so
    D = be.demod(1, same=False)
    for call in (D.same_read, lambda: D.same_get(0), lambda: D.same_stats(0)):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            call()
        assert ei.value.code == eng.EINVAL and "not enabled" in str(ei.value)
    keep_in, p_in = be.upload(stack(["eom"])[:, :1000])
    keep_out, p_out = be.zeros((1, 64, 2))
    D.process(p_in, 2000, 1000, p_out, 128, 64)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.same_enable()
    assert ei.value.code == eng.EINVAL and "before the first push" in str(ei.value)
    D.reset()
    with pytest.raises(eng.Nrsc5HipError):
        D.same_enable()                                                                  # a reset does not reopen it
    D.close()
    # beside RDS on one object: both decode, neither disturbs the other
    D = eng.FmDemod(1, lib_path=be.lib_path, same=True, rds=True)
    events, snap, stats, _ = session(be, D, stack(["header"]), [300000])
    assert D.rds_stats(0)["bits"] > 0 and D.rds_read() == []
    D.close()
    compare_session(events[0], snap[0], stats[0], sa.reference("header"), "header beside RDS")


def check_audio_untouched(be: Backend):
    """an existing fm_args case: the object without SAME and the object with it deliver the same audio bytes and clip counts, both are the float64
    audio model's within fm_checks' bound, and d through the stage hook is byte-equal"""
    names = ["lr80", "cnr40", "l1k"]
    x = fc.stack(names)
    off = be.demod(3, same=False)
    pcm0, clips0 = fc.run(be, off, x, [50000])
    keep, ptr = be.upload(x)
    d0 = off.stage_mpx(ptr, 2 * fa.N, fa.N)[0]
    off.close()
    on = be.demod(3, same=True)
    pcm1, clips1 = fc.run(be, on, x, [50000])
    d1 = on.stage_mpx(ptr, 2 * fa.N, fa.N)[0]
    want_bits = sm.WIN_BITS * sm.windows_total(sm.segments_total((fa.N + 1) // 2))
    st = on.same_stats(0)
    assert on.same_read() == [] and st["bits"] + st["seam_drops"] - st["seam_inserts"] == want_bits > 0     # a host without bursts: bits, no event
    on.close()
    assert pcm0.tobytes() == pcm1.tobytes() and np.array_equal(clips0, clips1) and d0.tobytes() == d1.tobytes()
    for c, name in enumerate(names):
        fc.compare(pcm0[c], clips0[c], name)


def expected_launches(n: int, chunks, same: bool):
    """kernel launches of a session from the definitions alone -> (audio path, SAME): per push the front end when a d sample is new, the pilot sums
    when a block is complete, the audio when an audio block is due, the kept tails always; with SAME the tone sums when a segment is new and,
    when a window was decided, decisions, framing and the kept c"""
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
        if same:
            r1 = sm.segments_total(m1)
            w1 = sm.windows_total(r1)
            extra += (r1 > r0) + 3 * (w1 > w0)
            r0, w0 = r1, w1
        m0, b0, a0 = m1, b1, a1
    return audio, extra


def check_launch_counts(be: Backend):
    """an fm_args case: the object without SAME launches what it did before SAME existed -- front, pilot sums, audio, kept tails: 4 for a session
    in one push -- and the object with SAME that plus its own launches"""
    names = ["lr80", "cnr40", "l1k"]
    x = fc.stack(names)
    plans = {"one": [], "two": [50000], "ones": [1] * 3000, "1080": [1080] * (fa.N // 1080 + 1)}
    off, on = be.demod(3, same=False), be.demod(3, same=True)
    assert off.launches() == 0 and on.launches() == 0
    for plan, chunks in plans.items():
        off.reset(); on.reset()
        fc.run(be, off, x, chunks)
        fc.run(be, on, x, chunks)
        audio, extra = expected_launches(fa.N, chunks, True)
        assert expected_launches(fa.N, chunks, False) == (audio, 0)
        print(f"{plan}: launches without SAME {off.launches()} (expected {audio}), with SAME {on.launches()} (expected {audio} + {extra})")
        assert off.launches() == audio, (plan, off.launches(), audio)
        assert on.launches() == audio + extra, (plan, on.launches(), audio, extra)
        if plan == "one":
            assert (audio, extra) == (4, 4)              # front + pilot + audio + keep; tone sums + decisions + framing + kept c
    keep, ptr = be.upload(x)
    before = on.launches()
    on.stage_same_tones(ptr, 2 * fa.N, fa.N)
    assert on.launches() == before                         # the stage hook runs a session of its own
    on.reset()
    assert on.launches() == 0
    off.close(); on.close()


# ------------------------------------------------------------------------------------------------------------------ framer level
def run_frames(be: Backend, name: str, pieces=None, burst_events: bool = True):
    bits, rst = sa.frame_cases()[name]
    D = be.demod(2, same_burst_events=burst_events)
    events = []
    if pieces is None:
        D.stage_same_frames([bits], channels=[1], reset_at=None if rst is None else [rst])
        events += D.same_read()
    else:                                                                      # the stream ends mid-byte and continues in the next call
        assert rst is None
        for a, b in zip([0] + pieces, pieces + [bits.size]):
            D.stage_same_frames([bits[a:b]], channels=[1])
            events += D.same_read()
    snap, stats, other = D.same_get(1), D.same_stats(1), D.same_stats(0)
    D.close()
    assert other == dict.fromkeys(eng.SAME_STATS, 0)                           # the channel not listed is untouched
    g = sa.frame_reference(name)
    got = split_events(events, 2) if pieces is None else [[], [event_key(e) for e in events]]
    want = model_events(g)
    if rst is not None:                                                        # what was reported in front of the reset comes first
        head = sm.Framer().push(bits[:rst])
        want = model_events(head) + want
    if not burst_events:
        want = [e for e in want if e[0] == "message"]
    assert got[0] == [] and got[1] == want, (name, got[1], want)
    assert snap == g.snapshot(), (name, snap, g.snapshot())
    if burst_events:
        assert stats == g.stats, (name, {k: (stats[k], g.stats[k]) for k in stats if stats[k] != g.stats[k]})
    else:
        assert {k: v for k, v in stats.items() if k != "events"} == {k: v for k, v in g.stats.items() if k != "events"} and stats["events"] == len(want)


def check_frames_case(be: Backend, name: str):
    run_frames(be, name)


def check_frames_in_pieces(be: Backend):
    run_frames(be, "header_then_eom", pieces=[24 + 100, 24 + 100 + 1, 24 + 128 + 8 * 20 + 3, 2000 + 5])
    run_frames(be, "majority", pieces=[700])
    run_frames(be, "two_of_three", burst_events=False)
    with pytest.raises(eng.Nrsc5HipError):
        be.demod(1, same_burst_events=2)


def check_frames_many_channels(be: Backend):
    """several channels in one call, listed out of order, one of them empty"""
    names = ["header_then_eom", "majority", "disagree"]
    D = be.demod(5)
    D.stage_same_frames([sa.frame_cases()[n][0] for n in names] + [np.zeros(0, np.uint8)], channels=[4, 0, 2, 3])
    events = split_events(D.same_read(), 5)
    for ch, name in zip([4, 0, 2], names):
        g = sa.frame_reference(name)
        assert events[ch] == model_events(g) and D.same_get(ch) == g.snapshot() and D.same_stats(ch) == g.stats, name
    assert events[1] == [] and events[3] == [] and D.same_stats(3)["bits"] == 0
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_same_frames([np.zeros(4, np.uint8)] * 2, channels=[1, 1])         # a channel listed twice
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_same_frames([np.zeros(4, np.uint8)], channels=[5])
    with pytest.raises(eng.Nrsc5HipError):
        D.stage_same_frames([np.zeros(4, np.uint8)], reset_at=[5])
    D.close()
