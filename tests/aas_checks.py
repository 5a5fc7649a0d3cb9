"""What the data-service tests compare (tests/test_aas_stage_cpu.py on the emulated build, tests/test_gpu_aas_stage.py on the gfx950 library): the events,
every counter and the SIG snapshot of nrsc5hip_stage_aas / nrsc5hip_stage_aas_frames / nrsc5hip_aas_feed against tests/aas_model.py on the packet lists of
tests/aas_args.py.  The model is itself compared with the unmodified reference (model_vs_reference).  Everything is equality: event for event (stream,
kind, port, seq, raw values, data), counter for counter.
The byte bound a call obeys, as include/nrsc5hip.h states it: 16 bytes of arena header per call, and per event 48 bytes and its data padded to 4."""
from __future__ import annotations

import ctypes

import numpy as np

from nrsc5_amd import engine as eng, synth
from tests import aas_args as aa, aas_model as am

_expected, _cache = {}, {}


def make_engine(lib_path, max_streams: int = 1):
    return eng.Engine(max_streams=max_streams, q15_capacity=200000, record_capacity=64, p1_slots=2, lib_path=lib_path)


def expected(name: str, fragments: bool = True):
    """-> {"packets": per packet [event], "stats", "sig"} of the whole list without a reset"""
    key = (name, fragments)
    if key not in _expected:
        lst = aa.get(name)
        per, m = am.run(lst["packets"], lst["lot_files"], fragments)
        _expected[key] = {"packets": per, "stats": dict(m.stats), "sig": m.sig()}
    return _expected[key]


def flat(per_packet, stream: int = 0):
    """the model's events as AasConsumer.raw holds them"""
    return [(stream, *ev) for pk in per_packet for ev in pk]


def bound(raw_events, calls: int = 1) -> int:
    return 16 * calls + sum(eng.AAS_EVENT_HEADER + (len(ev[-1]) + 3) // 4 * 4 for ev in raw_events)


def device_stats(C, stream: int = 0):
    st = C.stats(stream)
    return {k: st[k] for k in am.STATS}


def stage(C, targets, packets_per_stream):
    """one nrsc5hip_stage_aas call -> its raw events; the byte bound and the decoded events are checked on the way"""
    first, moved = len(C.raw), C.stats(targets[0])["d2h_bytes"]
    out = C.stage(targets, packets_per_stream)
    raw = C.raw[first:]
    assert C.stats(targets[0])["d2h_bytes"] - moved <= bound(raw)
    assert out == [(s, kind, eng.aas_event_fields(kind, port, seq, v, data)) for s, kind, port, seq, v, data in raw]
    return raw


def consumer(E, name: str, nstreams: int = 1, fragments: bool = True):
    return eng.AasConsumer(E, nstreams, lot_files=aa.get(name)["lot_files"], fragments=fragments)


def check_list_in_one_call(E, name: str):
    exp, pk = expected(name), aa.get(name)["packets"]
    C = consumer(E, name, 2)
    try:
        assert stage(C, [1], [pk]) == flat(exp["packets"], 1), name
        assert device_stats(C, 1) == exp["stats"], name
        assert C.sig(1) == exp["sig"], name
        assert device_stats(C, 0) == dict.fromkeys(am.STATS, 0) and C.sig(0) == []
    finally:
        C.close()


def check_packet_per_call(E, name: str):
    """a packet per call: every piece of state is carried from launch to launch"""
    exp, pk = expected(name), aa.get(name)["packets"]
    C = consumer(E, name)
    try:
        for k, p in enumerate(pk):
            assert stage(C, [0], [[p]]) == flat(exp["packets"][k:k + 1]), (name, k)
        assert device_stats(C) == exp["stats"] and C.sig(0) == exp["sig"], name
    finally:
        C.close()


def check_fragment_flag_off(E, name: str = "files"):
    """without the fragment flag no LOT_FRAGMENT event is written, and the counters count them all the same"""
    exp, pk = expected(name, fragments=False), aa.get(name)["packets"]
    assert exp["stats"]["lot_fragments"] == expected(name)["stats"]["lot_fragments"] >= 10
    assert not any(ev[0] == "lot_fragment" for p in exp["packets"] for ev in p)
    C = consumer(E, name, fragments=False)
    try:
        assert stage(C, [0], [pk]) == flat(exp["packets"])
        assert device_stats(C) == exp["stats"]
    finally:
        C.close()


def check_three_streams_in_one_call(E, names=("files", "lru", "headers"), targets=(3, 0, 2)):
    """three consumer streams with different lists in ONE call (their packets interleaved in the arena), the consumer streams not in the order of the list;
    two such calls, so that every state is carried from one multi-stream call into the next, and the second stream is empty in the first call"""
    C = eng.AasConsumer(E, 4, lot_files=16, fragments=True)
    try:
        pks, exps = [aa.get(n)["packets"] for n in names], [expected(n) for n in names]
        assert all(aa.get(n)["lot_files"] == 16 for n in names)
        cuts = [(0, 30), (0, 0), (0, 3)], [(30, len(pks[0])), (0, len(pks[1])), (3, len(pks[2]))]
        for part in cuts:
            got = stage(C, list(targets), [p[a:b] for p, (a, b) in zip(pks, part)])
            want = [ev for t, e, (a, b) in zip(targets, exps, part) for ev in flat(e["packets"][a:b], t)]
            assert got == want, (len(got), len(want))
        for t, e in zip(targets, exps):
            assert device_stats(C, t) == e["stats"] and C.sig(t) == e["sig"]
        assert device_stats(C, 1) == dict.fromkeys(am.STATS, 0)
    finally:
        C.close()


def check_reset(E, first: str = "files", second: str = "lru"):
    """nrsc5hip_aas_reset between two lists: table and files are gone, the counter is 1 again (the second list behaves as on a fresh stream), and the other
    stream keeps its state"""
    C = eng.AasConsumer(E, 2, lot_files=16, fragments=True)
    try:
        cut = 25
        pk = aa.get(first)["packets"]
        assert stage(C, [0, 1], [pk, pk[:cut]]) == flat(expected(first)["packets"]) + flat(expected(first)["packets"][:cut], 1)
        C.reset(0)
        assert C.sig(0) == [] and C.sig(1) == expected(first)["sig"]
        assert stage(C, [0, 1], [aa.get(second)["packets"], pk[cut:]]) == flat(expected(second)["packets"]) + flat(expected(first)["packets"][cut:], 1)
        assert C.sig(0) == expected(second)["sig"]
        total = {k: expected(first)["stats"][k] + expected(second)["stats"][k] for k in am.STATS}
        assert device_stats(C, 0) == total and device_stats(C, 1) == expected(first)["stats"]
    finally:
        C.close()


def check_arena_overflow(E, name: str = "files"):
    """an arena too small for the events of a call is NRSC5HIP_EOVERFLOW, never a silent drop; with the bound back in place the consumer works on"""
    pk = aa.get(name)["packets"]
    C = consumer(E, name)
    try:
        C.debug_arena(3 * eng.AAS_EVENT_HEADER)
        try:
            C.stage([0], [pk])
            raise AssertionError("no error")
        except eng.Nrsc5HipError as err:
            assert err.code == eng.EOVERFLOW
        assert C.events == [] and C.raw == []
        C.reset(0)
        one = expected(name)["packets"][2]                        # the first PSD-port packet: one event
        C.debug_arena(eng.AAS_EVENT_HEADER + (len(one[0][-1]) + 3) // 4 * 4)     # exactly that event fits
        assert [ev[1] for ev in C.stage([0], [pk[2:3]])] == ["psd"]
        C.debug_arena(0)
        C.reset(0)
        before = C.stats(0)
        assert stage(C, [0], [pk]) == flat(expected(name)["packets"])
        assert C.stats(0)["lot_files"] - before["lot_files"] == expected(name)["stats"]["lot_files"]
    finally:
        C.close()


def check_rejections(lib_path, name: str = "files"):
    """bad arguments are NRSC5HIP_EINVAL and leave state and counters as they were: the list goes on afterwards as if nothing had been tried"""
    E = make_engine(lib_path)
    C = eng.AasConsumer(E, 2, lot_files=16, fragments=True)
    P = eng.PsdConsumer(E, 2)
    try:
        pk, exp = aa.get(name)["packets"], expected(name)
        got = stage(C, [0], [pk[:20]])
        before, sig = C.stats(0), C.sig(0)
        lib = E.lib
        i32 = lambda v: np.array(v, dtype=np.int32)
        blob = eng.aas_packets(pk[:3])

        def stg(targets, nbytes, ptr=blob.ctypes.data):
            t, nb = i32(targets), i32(nbytes)
            ptrs = (ctypes.c_void_p * len(targets))(*([ptr] * len(targets)))
            return lib.nrsc5hip_stage_aas(C._h, len(targets), t.ctypes.data, ptrs, nb.ctypes.data, C._cb, None)

        recs = np.zeros(1, dtype=eng.RECORD_DTYPE)

        def feed(ids, targets, a=None, p=None):
            t, ii, counts = i32(targets), i32(ids), i32([0] * len(ids))
            ptrs = (ctypes.c_void_p * len(ids))(*([recs.ctypes.data] * len(ids)))
            return lib.nrsc5hip_aas_feed(C._h if a is None else a, P._h if p is None else p, E._h, len(ids), ii.ctypes.data, t.ctypes.data, ptrs, counts.ctypes.data,
                                         eng.MODE_FM, C._cb, None)

        out = ctypes.c_void_p()
        n, ns, buf = ctypes.c_uint(), ctypes.c_int(), (ctypes.c_uint8 * eng.AAS_SIG_MAX)()
        for rc in (stg([0, 0], [blob.size, blob.size]), stg([2], [blob.size]), stg([-1], [blob.size]), stg([0], [-1]), stg([0], [blob.size - 1]), stg([0], [5]),
                   stg([0], [blob.size], ptr=None), lib.nrsc5hip_stage_aas(C._h, 0, None, None, None, C._cb, None),
                   feed([0], [2]), feed([0], [-1]), feed([0, 0], [0, 0]), feed([0], [0], p=ctypes.c_void_p()), feed([5], [0]),
                   lib.nrsc5hip_aas_reset(C._h, 2), lib.nrsc5hip_aas_stats(C._h, 2, None), lib.nrsc5hip_aas_sig(C._h, -1, buf, ctypes.byref(n), ctypes.byref(ns)),
                   lib.nrsc5hip_aas_create(E._h, 1, 0, 0, ctypes.byref(out)), lib.nrsc5hip_aas_create(E._h, 1, eng.AAS_MAX_FILES + 1, 0, ctypes.byref(out)),
                   lib.nrsc5hip_aas_create(E._h, 0, 4, 0, ctypes.byref(out)), lib.nrsc5hip_aas_create(E._h, 1, 4, 2, ctypes.byref(out))):
            assert rc == eng.EINVAL
            assert C.stats(0) == before and C.sig(0) == sig and device_stats(C, 1) == dict.fromkeys(am.STATS, 0)
        # nothing to do is not an error
        assert feed([0], [0]) == 0 and stg([0], [0]) == 0
        assert eng.feed_aas_batch(E, C, P, [0], [None]) == [] and C.stage([0, 1], [[], []]) == []
        assert device_stats(C) == {k: before[k] for k in am.STATS}
        got += stage(C, [0], [pk[20:]])
        assert got == flat(exp["packets"]) and device_stats(C) == exp["stats"]
    finally:
        P.close()
        C.close()
        E.close()


# ---- the chain: frames -> index -> k_psd -> k_aas ----------------------------------------------------------------------------------------------------
CHAIN = ("carousel", "headers", "changes")


def chain_frames(name: str):
    if ("frames", name) not in _cache:
        pk = aa.carousel()["packets"] if name == "carousel" else aa.get(name)["packets"]
        _cache["frames", name] = (aa.psd_frames(pk, per_frame=2, span=150), [(p[0], p[1], bytes(p[2])) for p in pk])
    return _cache["frames", name]


def check_chain(E, targets=(2, 0, 1)):
    """three lists carried as PSD byte streams of three streams through nrsc5hip_stage_aas_frames, two calls: the events are the model's on the packets; the
    PSD consumer in front ends with the counters nrsc5hip_stage_psd_streams gives a consumer of its own on the same frames, whose packets are the lists;
    its packets did not cross (4 bytes per frame did), and the data services' counter obeys the bound"""
    A = eng.AasConsumer(E, 3, lot_files=16, fragments=True)
    P, Q = eng.PsdConsumer(E, 3), eng.PsdConsumer(E, 3)
    try:
        frames = [chain_frames(n)[0] for n in CHAIN]
        sent = [chain_frames(n)[1] for n in CHAIN]
        models = [am.AasModel(16, True) for _ in CHAIN]
        nframes = 0
        for part in (slice(0, 1), slice(1, None)):
            moved_a, moved_p = A.stats(0)["d2h_bytes"], P.stats(0)["d2h_bytes"]
            first = len(A.raw)
            fr = [f[part] for f in frames]
            got = A.stage_frames(P, list(targets), fr, [0, 0, 0])
            raw = A.raw[first:]
            assert got == [(s, kind, eng.aas_event_fields(kind, port, seq, v, data)) for s, kind, port, seq, v, data in raw]
            mine = Q.stage_streams(list(targets), fr, [0, 0, 0])
            want = []
            for t, m in zip(targets, models):
                for s, program, port, seq, data in mine:
                    if s == t:
                        want += [(t, *ev) for ev in m.push(port, seq, data, program)]
            assert raw == want, (len(raw), len(want))
            n = sum(len(f) for f in fr)
            nframes += n
            assert A.stats(0)["d2h_bytes"] - moved_a <= bound(raw) and P.stats(0)["d2h_bytes"] - moved_p == 4 * n
        for k, t in enumerate(targets):
            assert [(port, seq, data) for s, _, port, seq, data in Q.packets if s == t] == sent[k], CHAIN[k]
            assert {x: v for x, v in P.stats(t).items() if x != "d2h_bytes"} == {x: v for x, v in Q.stats(t).items() if x != "d2h_bytes"}
            assert device_stats(A, t) == models[k].stats and A.sig(t) == models[k].sig()
        assert P.packets == [] and models[0].stats["lot_files"] >= 2
    finally:
        A.close()
        P.close()
        Q.close()


def check_carousel(E, rounds: int = 3):
    """a carousel sent three times, a round per call: the bytes that cross are the files once plus the small events, not three times"""
    one = aa.carousel()["one"]
    frames = aa.psd_frames(one, per_frame=2, span=150)
    files = sum(len(b) for b in aa.carousel()["sent"].values())
    A = eng.AasConsumer(E, 1, lot_files=4, fragments=False)
    P = eng.PsdConsumer(E, 1)
    try:
        m, moved = am.AasModel(4, False), []
        for r in range(rounds):
            first, before = len(A.raw), A.stats(0)["d2h_bytes"]
            A.stage_frames(P, [0], [frames], [0])
            raw = A.raw[first:]
            assert raw == flat([m.push(*p[:3]) for p in one])                # (the stream is program 0's)
            moved.append(A.stats(0)["d2h_bytes"] - before)
            assert moved[-1] <= bound(raw)
            assert [ev[1] for ev in raw].count("lot") == (2 if r == 0 else 0)
        psd = sum(eng.AAS_EVENT_HEADER + (len(p[2]) + 3) // 4 * 4 for p in one if p[0] in am.PSD_PORTS)
        assert moved[0] >= files and all(x == 16 + psd for x in moved[1:]) and psd < files // 4, (moved, files, psd)
        assert m.stats["lot_duplicates"] == 2 * m.stats["lot_fragments"] // 3 and device_stats(A) == m.stats
    finally:
        A.close()
        P.close()


# ---- the unmodified reference ------------------------------------------------------------------------------------------------------------------------
def model_vs_reference(reflib, packets, lot_files: int = 16) -> int:
    """packet by packet through the reference's own output_aas_push (the PSD-port packets left out: they go to its ID3 parser) -> the events compared"""
    pk = [p for p in packets if p[0] not in am.PSD_PORTS]
    R = am.RefAas(reflib)
    try:
        ref = R.push(pk)
    finally:
        R.close()
    per, m = am.run(pk, lot_files, fragments=True)
    assert m.stats["pool_evictions"] == 0
    for k, (mine, theirs) in enumerate(zip(per, ref)):
        assert [am.ref_form(ev) for ev in mine] == theirs, k
    return sum(len(t) for t in ref)


E2E_FRAMES = 6


def e2e_stream() -> bytes:
    """program 0's PSD byte stream of the end-to-end capture: the SIG, an ID3 tag and a one-fragment file, three times over"""
    from tests import psd_args as pa
    body = b"\x89PNG one fragment of a station logo " + bytes(range(40))
    one = [(aa.SIG_PORT, 1, aa.STANDARD_SIG), (0x5100, 2, pa.id3_tag("A title", "An artist")),
           (aa.LOT_PORT_B, 3, aa.lot_packet(77, 0, body, aa.lot_header(len(body), aa.MIME_LOGO, b"logo.png")))]
    return b"".join(pa.hdlc(pa.aas_payload(*p)) for p in one) * 3


def capture():
    if "cap" not in _cache:
        _cache["cap"] = synth.fm_mp1_capture(E2E_FRAMES, seed=73, cfo_hz=-45.0, offset=640, snr_db=22, psd_stream=e2e_stream())
    return _cache["cap"]


def check_feed_end_to_end(lib_path, reflib, piece: int = 40):
    """the engine's records of the capture through nrsc5hip_aas_feed in pieces of `piece` records == the reference's events on the same IQ; the PSD consumer in
    front counts what nrsc5hip_psd_feed counts on the same records"""
    from tests import common
    cap = capture()
    R = am.RefAas(reflib)
    try:
        want = list(R.run_iq(cap.iq))
    finally:
        R.close()
    kinds = [e[0] for e in want]
    assert kinds.count("sig") == 1 and kinds.count("lot") == 1 and kinds.count("lot_fragment") >= 2 and kinds[0] == "sig", kinds     # on the reference alone
    E = eng.Engine(max_streams=1, q15_capacity=cap.iq.size // 4 + 200000, record_capacity=1024, p1_slots=16, lib_path=lib_path, p1_async=True, l2_feedback=True)
    A, P, Q = eng.AasConsumer(E, 2, lot_files=4, fragments=True), eng.PsdConsumer(E, 2), eng.PsdConsumer(E, 2)
    try:
        common.run_engine_streaming(E, 0, cap.iq, chunk=32768 * 8)
        recs = E.drain(0)
        for pos in range(0, len(recs), piece):
            first, moved = len(A.raw), A.stats(1)["d2h_bytes"]
            new = eng.feed_aas_batch(E, A, P, [0], [recs[pos:pos + piece]], targets=[1])
            assert A.stats(1)["d2h_bytes"] - moved <= bound(A.raw[first:]) and all(ev[0] == 1 for ev in new)
            eng.feed_psd_batch(E, Q, [0], [recs[pos:pos + piece]], targets=[1])
        assert [f for f in (am.ref_form(ev[1:]) for ev in A.raw) if f is not None] == want, (len(A.raw), len(want))
        assert [(ev[2], ev[3], ev[5]) for ev in A.raw if ev[1] == "psd"] == [(port, seq, data) for _, _, port, seq, data in Q.packets if port == 0x5100]
        assert {x: v for x, v in P.stats(1).items() if x != "d2h_bytes"} == {x: v for x, v in Q.stats(1).items() if x != "d2h_bytes"} and P.packets == []
        assert A.sig(1) == am.run([(aa.SIG_PORT, 0, aa.STANDARD_SIG)])[1].sig() and device_stats(A, 0) == dict.fromkeys(am.STATS, 0)
    finally:
        A.close()
        P.close()
        Q.close()
        E.close()
