"""What the PSD transport tests compare (tests/test_psd_stage_cpu.py on the emulated build, tests/test_gpu_psd_stage.py on the gfx950 library):
the packets and counters of nrsc5hip_stage_psd / nrsc5hip_psd_feed against tests/psd_model.py on the sessions of tests/psd_args.py.  The model is
fed from the ORACLE's L2 index (oracle/nrsc5_oracle_l2.c), not from the device's, and is itself compared with the unmodified reference's `l2aas`
records (model_vs_reference).  Everything is equality: packet for packet (stream, program, port, seq, bytes), counter for counter."""
from __future__ import annotations

import ctypes

import numpy as np

from nrsc5_amd import engine as eng
from tests import psd_args as pa, psd_model as pm

_expected = {}


def make_engine(lib_path, max_streams: int = 1):
    return eng.Engine(max_streams=max_streams, q15_capacity=200000, record_capacity=64, p1_slots=2, lib_path=lib_path)


def frames_of(s):
    """[(nbits, lc, bits)] frame by frame"""
    return [(nbits, lc, b) for nbits, lc, bits in s["pieces"] for b in bits]


def run_model(oracle, lib, name: str, reset_at=None):
    """the model over a session -> (per frame [(program, port, seq, data)], counters, PDUs kept per frame of the fixed-data session); reset_at: the frame in
    front of which the stream enters fine sync again (frame_reset: programs closed, fixed-data state cleared).  The fixed-data session's cut comes from the
    library's host restatement of process_fixed_data (pinned against the reference by tests/test_oracle_l2.py)."""
    s = pa.session(name)
    model = pm.PsdModel()
    H = eng.HdcConsumer(1, lib=lib) if name == "fixed" else None
    per_frame, kept = [], []
    for k, (nbits, lc, bits) in enumerate(frames_of(s)):
        if k == reset_at:
            model.reset()
            if H is not None:
                H.frame_reset(0)
        if H is None:
            idx, by = oracle.l2_index(bits)
            per_frame.append(model.push_frame(idx, by))
            continue
        fr, by = oracle.l2_index_struct(bits)
        b = np.frombuffer(by, dtype=np.uint8)
        cut = eng.L2Frame.from_buffer_copy(fr)
        n = lib.nrsc5hip_l2_apply_audio_end(ctypes.byref(cut), H.fixed_audio_end(0, lc, b[:fr.nbytes]))
        assert n >= 0
        kept.append(n)
        per_frame.append(model.push_frame(eng.l2_frame_to_dict(cut), b))
    if H is not None:
        H.close()
    return per_frame, dict(model.stats), kept


def expected(oracle, lib, name: str):
    """-> {"frames": per frame [(program, port, seq, data)], "stats": the model's counters, "kept"} of the whole session without a reset"""
    if name not in _expected:
        per_frame, stats, kept = run_model(oracle, lib, name)
        if name == "fixed":
            assert kept[0] == 5 and kept[-1] < 5, kept                    # the cut really removes PDUs that carry PSD
        _expected[name] = {"frames": per_frame, "stats": stats, "kept": kept}
    return _expected[name]


def bound(packets, nstreams: int = 1) -> int:
    """what a feed may move to the host: its packets + 16 bytes each + 256 bytes per listed stream"""
    return sum(len(p[-1]) + 16 for p in packets) + 256 * nstreams


def flat(per_frame, stream: int = 0):
    return [(stream,) + p for fr in per_frame for p in fr]


def device_stats(P, stream: int = 0):
    st = P.stats(stream)
    return {k: st[k] for k in pm.STATS}


def model_vs_reference(oracle, lib, reflib, name: str) -> int:
    """the model's packets == the reference's l2aas records, frame by frame, one reference session; -> packets"""
    s = pa.session(name)
    exp = expected(oracle, lib, name)
    logs = reflib.l2_frames([b for _, _, b in frames_of(s)])
    n = 0
    for k, (log, mine) in enumerate(zip(logs, exp["frames"])):
        # (a packet shorter than port + seq, which the reference hands on and reads past, is dropped by the rules: a stated deviation)
        ref_pkts = [v["data"] for kind, v in log if kind == "l2aas" and len(v["data"]) >= 4]
        assert [pm.packet_bytes(p) for p in mine] == ref_pkts, (name, k)
        n += len(ref_pkts)
    return n


def check_session_in_one_call(E, oracle, name: str):
    """every piece of the session in one call (a session of one frame length: the whole session)"""
    s, exp = pa.session(name), expected(oracle, E.lib, name)
    P = eng.PsdConsumer(E, 2)
    try:
        total = 0
        for nbits, lc, bits in s["pieces"]:
            first, moved = len(P.packets), P.stats(1)["d2h_bytes"]
            total += P.stage(1, np.stack(bits), lc)
            if name != "fixed":
                assert P.stats(1)["d2h_bytes"] - moved <= bound(P.packets[first:]), name
        assert P.packets == flat(exp["frames"], 1), (name, len(P.packets))
        assert total == len(P.packets)
        assert device_stats(P, 1) == exp["stats"], name
        assert device_stats(P, 0) == dict.fromkeys(pm.STATS, 0)
    finally:
        P.close()


def check_frame_per_call(E, oracle, name: str):
    """one frame per call: each call delivers exactly the packets the model closes in that frame, and -- without fixed data -- moves no more than the packets
    (their bytes + 16 each) + 256 bytes to the host: the frame never crosses"""
    s, exp = pa.session(name), expected(oracle, E.lib, name)
    P = eng.PsdConsumer(E, 1)
    try:
        moved = 0
        for (nbits, lc, bits), want in zip(frames_of(s), exp["frames"]):
            first = len(P.packets)
            P.stage(0, bits, lc)
            got = P.packets[first:]
            assert got == [(0,) + p for p in want], (name, len(got), len(want))
            now = P.stats(0)["d2h_bytes"]
            if name != "fixed":
                assert now - moved <= bound(got), (name, now - moved)
            moved = now
        assert device_stats(P) == exp["stats"], name
    finally:
        P.close()


def check_three_streams_in_one_call(E, oracle, names=("dense1", "am", "overflow8213"), targets=(3, 0, 2)):
    """three consumer streams carrying different sessions in ONE call (nrsc5hip_stage_psd_streams: one index launch over all frames, one k_psd launch of three
    workgroups sharing the arena), the consumer streams not in the order of the list; the sessions in two such calls, so that every state is carried from a
    multi-stream call into the next.  Per call: all of targets[0] first, each stream's packets in order, and the byte bound; at the end every counter."""
    P = eng.PsdConsumer(E, 4)
    try:
        frames = [frames_of(pa.session(n)) for n in names]
        exps = [expected(oracle, E.lib, n) for n in names]
        cuts = [(0, (len(f) + 1) // 2) for f in frames], [((len(f) + 1) // 2, len(f)) for f in frames]
        seen = []
        for part in cuts:
            moved = P.stats(0)["d2h_bytes"]
            got = P.stage_streams(targets, [np.stack([b for _, _, b in f[a:b]]) for f, (a, b) in zip(frames, part)], [f[0][1] for f in frames])
            want = [(t,) + p for t, e, (a, b) in zip(targets, exps, part) for fr in e["frames"][a:b] for p in fr]
            assert got == want, (len(got), len(want))
            seen.append(len({p[0] for p in got}))
            assert P.stats(0)["d2h_bytes"] - moved <= bound(got, 3)
        assert seen == [2, 3]                                                # streams that deliver in each call (the overflow session: behind its long frame only)
        for t, e in zip(targets, exps):
            assert device_stats(P, t) == e["stats"]
        assert device_stats(P, 1) == dict.fromkeys(pm.STATS, 0)
    finally:
        P.close()


def check_to_fine_reset(E, oracle):
    """what a NRSC5HIP_REC_TO_FINE record does, with HDLC frames open in every program: k_psd's reset job in front of a frame (dense2), the fixed-data state
    cleared with it (fixed: the cut, two PDUs deep by then, is back at the frame's end), and a record that announces no frame (dense3: the reset stands behind
    the last frame of the first call) -- three streams in one call, against the model with frame_reset at those places"""
    P = eng.PsdConsumer(E, 3)
    try:
        names, resets = ("dense2", "fixed", "dense3"), (2, 5, 2)
        frames = [frames_of(pa.session(n)) for n in names]
        models = [run_model(oracle, E.lib, n, r) for n, r in zip(names, resets)]
        plain = [expected(oracle, E.lib, n) for n in names]
        assert models[1][2][4] < 5 and models[1][2][5] == 5 and plain[1]["kept"][5] < 5   # the fixed-data state really starts over
        for k in (0, 2):
            assert models[k][1]["delivered"] < plain[k]["stats"]["delivered"]    # the reset costs packets: frames were open
        assert models[1][0][5] and models[1][0] != plain[1]["frames"]           # fixed: other packets, the PDUs behind the old cut are walked again
        take = [(0, len(frames[0])), (0, len(frames[1])), (0, 2)]
        got = P.stage_streams([0, 1, 2], [np.stack([b for _, _, b in f[a:b]]) for f, (a, b) in zip(frames, take)], [0, 0, 0], reset_at=resets)
        got += P.stage_streams([2], [np.stack([b for _, _, b in frames[2][2:]])], [0])
        for k, (per_frame, stats, _) in enumerate(models):
            assert [p for p in got if p[0] == k] == flat(per_frame, k), names[k]
            assert device_stats(P, k) == stats, names[k]
    finally:
        P.close()


def check_reset_mid_frame(E, oracle, name: str = "dense2", after: int = 2):
    """nrsc5hip_psd_reset between two frames, with HDLC frames open in every program: what the model gives with a frame_reset there"""
    s = pa.session(name)
    model = pm.PsdModel()
    P = eng.PsdConsumer(E, 1)
    try:
        want = []
        for k, (nbits, lc, bits) in enumerate(frames_of(s)):
            if k == after:
                assert sum(1 for i in model.idx if i > 0) >= 3           # frames are open
                model.reset()
                P.reset(0)
            idx, by = oracle.l2_index(bits)
            want += model.push_frame(idx, by)
            P.stage(0, bits, lc)
        assert P.packets == [(0,) + p for p in want]
        assert device_stats(P) == model.stats
        assert len(want) < len(flat(expected(oracle, E.lib, name)["frames"]))  # the reset cost packets: the scene tells the two apart
    finally:
        P.close()


def check_rejections(lib_path, oracle, name: str = "dense3"):
    """nrsc5hip_psd_feed / nrsc5hip_stage_psd refuse bad arguments with NRSC5HIP_EINVAL and leave the state and the counters as they were: the session goes on
    afterwards as if nothing had been tried"""
    E = make_engine(lib_path, max_streams=2)
    P = eng.PsdConsumer(E, 2)
    try:
        fr = frames_of(pa.session(name))
        exp = expected(oracle, E.lib, name)
        for nbits, lc, bits in fr[:2]:
            P.stage(0, bits, lc)
        before, packets = P.stats(0), list(P.packets)
        recs = np.zeros(3, dtype=eng.RECORD_DTYPE)                        # three blocks, one P1 frame (the ring slot holds zeros: no PDU)
        recs["flags"] = eng.REC_PROCESSED
        recs["flags"][1] |= eng.REC_P1
        lib = E.lib

        def feed(ids, ptr, count, mode=eng.MODE_FM, targets=None):
            a = np.array(ids, dtype=np.int32)
            t = None if targets is None else np.array(targets, dtype=np.int32)
            ptrs = (ctypes.c_void_p * len(ids))(*([ptr] * len(ids)))
            counts = np.array([count] * len(ids), dtype=np.int32)
            return lib.nrsc5hip_psd_feed(P._h, E._h, len(ids), a.ctypes.data, None if t is None else t.ctypes.data, ptrs, counts.ctypes.data, mode, P._cb, None)

        def streams(targets, reset=None):
            n = len(targets)
            i32 = lambda v: np.array(v, dtype=np.int32)
            ptrs = (ctypes.c_void_p * n)(*([fr[2][2].ctypes.data] * n))
            tg, nb, nf, lc, rs = i32(targets), i32([146176] * n), i32([1] * n), i32([0] * n), None if reset is None else i32(reset)
            return lib.nrsc5hip_stage_psd_streams(P._h, E._h, n, tg.ctypes.data, ptrs, nb.ctypes.data, nf.ctypes.data, lc.ctypes.data,
                                                  None if rs is None else rs.ctypes.data, P._cb, None)

        p = recs.ctypes.data
        bad = recs.copy()
        bad["p1_slot"] = 99                                               # a slot the engine lacks
        for rc in (feed([2], p, 3), feed([-1], p, 3), feed([0], p, 3, targets=[2]), feed([0], p, 3, targets=[-1]), feed([0], None, 3), feed([0], p, -1),
                   feed([0], p, 3, mode=2), feed([0], bad.ctypes.data, 3), feed([0, 1], p, 3, targets=[0, 0]),
                   lib.nrsc5hip_psd_feed(P._h, E._h, 1, None, None, None, None, eng.MODE_FM, P._cb, None),
                   lib.nrsc5hip_stage_psd(P._h, E._h, 0, None, 146176, 1, 0, P._cb, None),
                   lib.nrsc5hip_stage_psd(P._h, E._h, 2, fr[2][2].ctypes.data, 146176, 1, 0, P._cb, None),
                   lib.nrsc5hip_stage_psd(P._h, E._h, 0, fr[2][2].ctypes.data, 146176, 0, 0, P._cb, None),
                   lib.nrsc5hip_stage_psd(P._h, E._h, 0, fr[2][2].ctypes.data, 146176, 1, 3, P._cb, None),
                   streams([0, 0]), streams([0, 1], reset=[0, 2]), streams([0, 2])):
            assert rc == eng.EINVAL
            after = P.stats(0)
            assert after == before and P.packets == packets
        # nothing to do is not an error; frames without PDUs deliver nothing and walk nothing
        assert lib.nrsc5hip_psd_feed(P._h, E._h, 0, None, None, None, None, eng.MODE_FM, P._cb, None) == 0
        assert feed([0], p, 0) == 0 and feed([0], None, 0) == 0
        assert eng.feed_psd_batch(E, P, [0], [recs]) == []
        assert device_stats(P) == {k: before[k] for k in pm.STATS}
        # ... and the session goes on where it was
        for nbits, lc, bits in fr[2:]:
            P.stage(0, bits, lc)
        assert P.packets == flat(exp["frames"]) and device_stats(P) == exp["stats"]
    finally:
        P.close()
        E.close()
