"""What the SIS tests compare (tests/test_sis_stage_cpu.py on the emulated build, tests/test_gpu_sis_stage.py on the gfx950 library): the events, the
snapshot and every counter of nrsc5hip_stage_sis / nrsc5hip_sis_feed against tests/sis_model.py on the frame sets of tests/sis_args.py.  The model is itself
compared with the unmodified reference (model_vs_reference_*).  Everything is equality: event for event (stream, frame, kind, raw values, encoding, raw
text), counter for counter."""
from __future__ import annotations

import ctypes

import numpy as np

from nrsc5_amd import engine as eng, synth
from tests import sis_args as sa, sis_model as sm

_expected, _cache = {}, {}
CAPTURE_FRAMES = 6


def make_engine(lib_path, max_streams: int = 1):
    return eng.Engine(max_streams=max_streams, q15_capacity=200000, record_capacity=64, p1_slots=2, lib_path=lib_path)


def expected(name: str):
    """-> {"frames": per frame [event], "stats", "info"} of the whole set without a reset"""
    if name not in _expected:
        per, m = sm.run(sa.frames(name))
        _expected[name] = {"frames": per, "stats": dict(m.stats), "info": m.info()}
    return _expected[name]


def flat(per_frame, stream: int = 0, first: int = 0):
    """the model's events as SisConsumer.raw holds them; first: index of per_frame[0] in the call's list"""
    return [(stream, first + k, *ev) for k, fr in enumerate(per_frame) for ev in fr]


def bound(raw_events) -> int:
    """what a call may move to the host: 16 bytes of arena header, and per event its header and its text padded to 4"""
    return 16 + sum(eng.SIS_EVENT_HEADER + (len(ev[-1]) + 3) // 4 * 4 for ev in raw_events)


def device_stats(C, stream: int = 0):
    st = C.stats(stream)
    return {k: st[k] for k in sm.STATS}


def stage(C, targets, frames_per_stream, reset_at=None):
    """one nrsc5hip_stage_sis call -> its raw events; the byte bound and the decoded events are checked on the way"""
    first, moved = len(C.raw), C.stats(targets[0])["d2h_bytes"]
    out = C.stage(targets, frames_per_stream, reset_at)
    raw = C.raw[first:]
    assert C.stats(targets[0])["d2h_bytes"] - moved <= bound(raw)
    assert out == [(s, f, kind, eng.sis_event_fields(kind, v, enc, data)) for s, f, kind, v, enc, data in raw]
    return raw


def check_set_in_one_call(E, name: str):
    exp, fr = expected(name), sa.frames(name)
    C = eng.SisConsumer(E, 2)
    try:
        assert stage(C, [1], [fr]) == flat(exp["frames"], 1), name
        assert device_stats(C, 1) == exp["stats"], name
        assert C.info(1) == exp["info"], name
        assert device_stats(C, 0) == dict.fromkeys(sm.STATS, 0) and C.info(0) == sm.SisModel().info()
    finally:
        C.close()


def check_rewritten_lengths(E):
    """a frame 0 with the same seq rewrites the length of a displayed message / slogan / alert to 255 / 127 / 511: the snapshot holds what the buffers hold
    (190 / 95 / 381 bytes, the control data within the alert) and every field behind the texts is what it was"""
    fr, n = sa.frames("relength"), len(sa.longest())
    per, m = sm.run(fr)
    assert (m.msg_len, m.slogan_len, m.alert_len, m.alert_cnt_len) == sa.RELENGTH + (63,) and m.msg_displayed and m.slogan_displayed and m.alert_displayed
    C = eng.SisConsumer(E, 1)
    try:
        assert stage(C, [0], [fr[:n + 2]]) == flat(per[:n + 2])
        before = C.info(0)
        assert stage(C, [0], [fr[n + 2:]]) == flat(per[n + 2:])
        s = eng.SisInfo()
        assert C.lib.nrsc5hip_sis_get(C._h, 0, ctypes.byref(s)) == 0
        assert (s.message_len, s.slogan_len, s.alert_len, s.alert_cnt_len) == (190, 95, 381, 63)
        assert (s.message_enc, s.slogan_enc, s.alert_enc, s.have_location, s.n_audio, s.n_data) == (0, 0, 0, 1, 1, 1)
        after = C.info(0)
        assert after == m.info()
        for key in ("country", "fcc", "name", "location", "audio_services", "data_services"):
            assert after[key] == before[key], key
        # the first bytes are the rewriting frames', the rest of each text is the displayed item's
        assert after["message"] == "MSG!" + before["message"][4:] and len(after["message"]) == 190
        assert after["slogan"] == "SLOGN" + before["slogan"][5:] and len(after["slogan"]) == 95
        assert after["alert_control_data"] == b"\x01\x02\x03" + before["alert_control_data"][3:] and after["alert"] == before["alert"]
        assert device_stats(C) == m.stats
    finally:
        C.close()


def check_pieces(E, name: str, piece: int):
    """the set in calls of `piece` frames: piece 1 is a frame per call, 63 / 64 / 65 / 129 put the chunk boundary of the frame-parallel phase everywhere"""
    exp, fr = expected(name), sa.frames(name)
    C = eng.SisConsumer(E, 1)
    try:
        for p in range(0, len(fr), piece):
            assert stage(C, [0], [fr[p:p + piece]]) == flat(exp["frames"][p:p + piece]), (name, piece, p)
        assert device_stats(C) == exp["stats"] and C.info(0) == exp["info"], (name, piece)
    finally:
        C.close()


def check_three_streams_in_one_call(E, names=("schedule", "random2", "schedule1"), targets=(3, 0, 2)):
    """three consumer streams with different sets in ONE call, the consumer streams not in the order of the list; two such calls, so that every state
    is carried from one multi-stream call into the next, and the second stream is empty in the first call"""
    C = eng.SisConsumer(E, 4)
    try:
        frs, exps = [sa.frames(n) for n in names], [expected(n) for n in names]
        cuts = [(0, 70), (0, 0), (0, 33)], [(70, len(frs[0])), (0, len(frs[1])), (33, len(frs[2]))]
        for part in cuts:
            got = stage(C, list(targets), [f[a:b] for f, (a, b) in zip(frs, part)])
            want = [ev for t, e, (a, b) in zip(targets, exps, part) for ev in flat(e["frames"][a:b], t)]
            assert got == want, (len(got), len(want))
        for t, e in zip(targets, exps):
            assert device_stats(C, t) == e["stats"] and C.info(t) == e["info"]
        assert device_stats(C, 1) == dict.fromkeys(sm.STATS, 0)
    finally:
        C.close()


def mid_item_frame(name: str = "schedule") -> int:
    """a frame of the set in front of which a station message is half received: resetting there costs that message"""
    per = expected(name)["frames"]
    k = next(k for k, fr in enumerate(per) if any(ev[0] == "station_message" for ev in fr))
    return k - 1


def check_reset_at(E, name: str = "schedule"):
    """what a NRSC5HIP_REC_TO_FINE record does: the state pids_init leaves, in front of a frame in the middle of an item (stream 0), in front of the first
    frame of a later call (stream 1), and behind the last frame of a call (stream 2: a record that announces no frame) -- three streams in one call"""
    fr, plain = sa.frames(name), expected(name)
    r = mid_item_frame(name)
    models = [sm.run(fr, r), sm.run(fr, 40), sm.run(fr, 40)]
    assert models[0][0] != plain["frames"]
    assert [ev[0] for f in models[0][0][r:r + 3] for ev in f].count("station_message") == 0 and any(ev[0] == "station_message" for ev in plain["frames"][r + 1])
    C = eng.SisConsumer(E, 3)
    try:
        got = stage(C, [0, 1, 2], [fr, fr[:40], fr[:40]], reset_at=[r, -1, 40])
        got += stage(C, [1, 2], [fr[40:], fr[40:]], reset_at=[0, None])
        for k, (per, m) in enumerate(models):
            mine = [ev for ev in got if ev[0] == k]
            want = flat(per, k) if k == 0 else flat(per[:40], k) + flat(per[40:], k)
            assert mine == want, k
            assert device_stats(C, k) == m.stats and C.info(k) == m.info(), k
        # the stations are known again behind the reset: the state really started over
        assert sum(1 for ev in got if ev[0] == 1 and ev[2] == "station_id") > sum(1 for f in plain["frames"] for ev in f if ev[0] == "station_id")
    finally:
        C.close()


def check_reset_mid_item(E, name: str = "schedule"):
    """nrsc5hip_sis_reset between two calls, a station message half received"""
    fr = sa.frames(name)
    r = mid_item_frame(name)
    per, m = sm.run(fr, r)
    C = eng.SisConsumer(E, 1)
    try:
        got = stage(C, [0], [fr[:r]])
        C.reset(0)
        assert C.info(0) == sm.SisModel().info()
        got += stage(C, [0], [fr[r:]])
        assert got == flat(per[:r]) + flat(per[r:])
        assert device_stats(C) == m.stats and C.info(0) == m.info()
        assert got != flat(expected(name)["frames"][:r]) + flat(expected(name)["frames"][r:])
    finally:
        C.close()


def check_arena_overflow(E, name: str = "schedule"):
    """an arena too small for the events of a call is NRSC5HIP_EOVERFLOW, never a silent drop; with the bound back in place the consumer works on"""
    fr = sa.frames(name)
    C = eng.SisConsumer(E, 1)
    try:
        C.debug_arena(3 * eng.SIS_EVENT_HEADER)
        try:
            C.stage([0], [fr])
            raise AssertionError("no error")
        except eng.Nrsc5HipError as err:
            assert err.code == eng.EOVERFLOW
        assert C.events == [] and C.raw == []
        C.debug_arena(2 * (eng.SIS_EVENT_HEADER + 8))           # exactly the first frame's two events (station id, short name) fit
        assert len(C.stage([0], [fr[:1]])) == 0                   # (known since the first call: nothing to report)
        C.reset(0)
        assert [ev[2] for ev in C.stage([0], [fr[:1]])] == ["station_id", "station_name"]
        C.debug_arena(0)
        C.reset(0)
        assert stage(C, [0], [fr]) == flat(expected(name)["frames"])
    finally:
        C.close()


def check_rejections(lib_path, name: str = "schedule"):
    """bad arguments are NRSC5HIP_EINVAL and leave state and counters as they were: the set goes on afterwards as if nothing had been tried"""
    E = make_engine(lib_path)
    C = eng.SisConsumer(E, 2)
    try:
        fr, exp = sa.frames(name), expected(name)
        got = stage(C, [0], [fr[:50]])
        before, info = C.stats(0), C.info(0)
        lib = E.lib
        recs = np.zeros(3, dtype=eng.RECORD_DTYPE)
        recs["flags"] = eng.REC_PROCESSED | eng.REC_PIDS | eng.REC_TO_FINE
        i32 = lambda v: np.array(v, dtype=np.int32)

        def feed(targets, ptr, count):
            t, counts = i32(targets), i32([count] * len(targets))
            ptrs = (ctypes.c_void_p * len(targets))(*([ptr] * len(targets)))
            return lib.nrsc5hip_sis_feed(C._h, len(targets), t.ctypes.data, ptrs, counts.ctypes.data, C._cb, None)

        def stg(targets, nframes, reset=None, ptr=fr.ctypes.data):
            t, nf, rs = i32(targets), i32(nframes), None if reset is None else i32(reset)
            ptrs = (ctypes.c_void_p * len(targets))(*([ptr] * len(targets)))
            return lib.nrsc5hip_stage_sis(C._h, len(targets), t.ctypes.data, ptrs, nf.ctypes.data, None if rs is None else rs.ctypes.data, C._cb, None)

        p = recs.ctypes.data
        for rc in (feed([2], p, 3), feed([-1], p, 3), feed([0, 0], p, 3), feed([0], None, 3), feed([0], p, -1), feed([1, 0], None, 1),
                   lib.nrsc5hip_sis_feed(C._h, 1, None, None, None, C._cb, None), lib.nrsc5hip_sis_feed(C._h, -1, None, None, None, C._cb, None),
                   stg([0, 0], [1, 1]), stg([2], [1]), stg([0], [-1]), stg([0], [2], reset=[3]), stg([0], [2], ptr=None),
                   lib.nrsc5hip_stage_sis(C._h, 0, None, None, None, None, C._cb, None), lib.nrsc5hip_sis_reset(C._h, 2), lib.nrsc5hip_sis_stats(C._h, 2, None),
                   lib.nrsc5hip_sis_get(C._h, -1, None)):
            assert rc == eng.EINVAL
            assert C.stats(0) == before and C.info(0) == info and device_stats(C, 1) == dict.fromkeys(sm.STATS, 0)
        # nothing to do is not an error
        assert lib.nrsc5hip_sis_feed(C._h, 0, None, None, None, C._cb, None) == 0 and feed([0], p, 0) == 0 and feed([0], None, 0) == 0
        assert eng.feed_sis_batch(C, [0, 1], [None, np.zeros(0, dtype=eng.RECORD_DTYPE)]) == []
        assert C.stats(0) == before
        got += stage(C, [0], [fr[50:]])
        assert got == flat(exp["frames"][:50]) + flat(exp["frames"][50:], first=0) and device_stats(C) == exp["stats"]
    finally:
        C.close()
        E.close()


# ---- the unmodified reference ------------------------------------------------------------------------------------------------------------------------
def capture():
    """a 6-frame MP1 capture whose PIDS frames are the schedule without the never-complete lengths"""
    if "cap" not in _cache:
        _cache["cap"] = synth.fm_mp1_capture(CAPTURE_FRAMES, seed=71, cfo_hz=31.0, offset=500, snr_db=22, pids=sa.schedule(0, never_complete=False))
    return _cache["cap"]


def reference_on_capture(reflib, iq=None, key="ref"):
    """the reference on the capture -> (the frames its pids_frame_push was handed, its public-API SIS events); the ctypes layout of the event is checked by
    requiring its station-id events to equal the harness's `station` records"""
    if key not in _cache:
        iq = capture().iq if iq is None else iq
        log, _, _ = reflib.run(iq)
        pushed = np.stack([v["bits"] for k, v in log if k == "pids"])
        stations = [("station_id", v["country"].encode(), v["fcc"]) for k, v in log if k == "station"]
        R = sm.RefSis(reflib)
        try:
            events = list(R.run_iq(iq))
        finally:
            R.close()
        assert [e for e in events if e[0] == "station_id"] == stations and stations
        _cache[key] = (pushed, events)
    return _cache[key]


def model_vs_reference_capture(reflib):
    pushed, events = reference_on_capture(reflib)
    per, m = sm.run(pushed)
    assert [sm.ref_form(ev) for fr in per for ev in fr] == events
    # on the reference alone: enough frames reach it, and every kind of event fires
    assert m.stats["crc_good"] >= 60, m.stats
    assert {e[0] for e in events} == set(eng.SIS_KINDS[1:]), {e[0] for e in events}
    assert ("alert", None, None) in events and any(e[0] == "alert" and e[1] is not None for e in events)
    return m


def model_vs_reference_frames(reflib, frames):
    """frame sets without a capture: through the reference's own pids_frame_push, frame by frame"""
    R = sm.RefSis(reflib)
    try:
        ref = R.push_frames(frames)
    finally:
        R.close()
    per, _ = sm.run(frames)
    for k, (mine, theirs) in enumerate(zip(per, ref)):
        assert [sm.ref_form(ev) for ev in mine] == theirs, k
    return sum(len(t) for t in ref)


def check_feed_end_to_end(lib_path, reflib, piece: int = 3):
    """the engine's records of the capture through nrsc5hip_sis_feed in pieces of `piece` records == the reference's events on the same IQ; the CRC-good
    counter is the number of REC_PIDS_CRC flags; the bytes each call moves are bounded by its events"""
    from tests import common
    cap = capture()
    _, want = reference_on_capture(reflib)
    E = eng.Engine(max_streams=1, q15_capacity=cap.iq.size // 4 + 200000, record_capacity=1024, p1_slots=16, lib_path=lib_path, p1_async=True, l2_feedback=True)
    C = eng.SisConsumer(E, 2)
    try:
        common.run_engine_streaming(E, 0, cap.iq, chunk=32768 * 8)
        recs = E.drain(0)
        for pos in range(0, len(recs), piece):
            first, moved = len(C.raw), C.stats(1)["d2h_bytes"]
            part = recs[pos:pos + piece]
            new = eng.feed_sis_batch(C, [1], [part])
            raw = C.raw[first:]
            assert C.stats(1)["d2h_bytes"] - moved <= bound(raw)
            npids = int(np.sum((part["flags"] & eng.REC_PIDS) != 0))
            assert all(ev[0] == 1 and 0 <= ev[1] < npids for ev in new)
        assert [sm.ref_form(ev[2:]) for ev in C.raw] == want, (len(C.raw), len(want))
        fl = recs["flags"]
        st = C.stats(1)
        assert st["frames"] == int(np.sum((fl & eng.REC_PIDS) != 0)) and st["crc_good"] == int(np.sum(((fl & eng.REC_PIDS) != 0) & ((fl & eng.REC_PIDS_CRC) != 0))) >= 60
        assert st["events"] == len(want) and C.info(1)["name"] is not None and device_stats(C, 0) == dict.fromkeys(sm.STATS, 0)
    finally:
        C.close()
        E.close()
