"""`-m "not gpu"`: nrsc5hip_hdc_feed (eng.feed_hdc_batch) on the CPU-emulated twin -- block records of many streams replayed into the
batch HDC consumer in one native call.  Every comparison is against the NRSC5_EVENT_HDC sequence of the UNMODIFIED reference on
the same IQ (reflib.run(..., taps=ref.TAP_HDC)): program, byte count, flags and payload, in order; the Python per-record loop
eng.feed_hdc must give the same list."""
import ctypes

import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth
from oracle import ref
from tests import common, engine_checks as ec, trim_checks as tc

_cache = {}


def _reference_hdc(reflib, iq, mode=ref.MODE_FM):
    log, _, _ = reflib.run(iq, mode=mode, taps=ref.TAP_HDC)
    return [(v["program"], v["count"], v["flags"], bytes(v["data"])) for k, v in log if k == "hdc"]


def _events(H, stream):
    return [(p, c, f, d) for (s, p, c, f, d) in H.events if s == stream]


def _mp1_caps():
    """the two captures of engine_checks.check_l2_index_fused, one L1 frame longer: at its 2 frames the reference delivers 32 HDC packets on
    the first (cfo 25 Hz, offset 400) and none on the second (cfo -310 Hz, offset 3100: its first P1 frame arrives with too few blocks
    left behind it for output_advance), so the second misses the floor of 32 packets per capture; at 3 frames it delivers 64 and 32 --
    the shortest length at which both reach the floor"""
    if "mp1" not in _cache:
        _cache["mp1"] = [synth.fm_mp1_capture(3, seed=61 + k, cfo_hz=c, offset=o, snr_db=22) for k, (c, o) in enumerate([(25.0, 400), (-310.0, 3100)])]
    return _cache["mp1"]


def _mp1_reference(reflib):
    if "mp1_ref" not in _cache:
        _cache["mp1_ref"] = [_reference_hdc(reflib, c.iq) for c in _mp1_caps()]
        for exp in _cache["mp1_ref"]:
            assert len(exp) >= 32, "capture yields too few HDC packets to mean anything"
    return _cache["mp1_ref"]


def _engine(lib, caps, p1_async, am=False):
    n = len(caps)
    q15 = 400000 if am else max(c.iq.size // (4 if c.iq.dtype == np.uint8 else 2) for c in caps) + 200000
    E = eng.Engine(max_streams=n, q15_capacity=q15, record_capacity=1024, p1_slots=16,
                   lib_path=lib, p1_async=p1_async, l2_feedback=True, am_enable=am)
    if am:
        for k in range(n):
            E.set_mode(k, eng.MODE_AM)
    return E


def _run(E, caps, chunk=32768 * 8):
    """-> the records of every stream, all frames still in the rings (p1_slots = 16)"""
    recs = []
    for k, c in enumerate(caps):
        common.run_engine_streaming(E, k, c.iq, chunk=chunk)
        recs.append(E.drain(k))
    return recs


@pytest.fixture(scope="module")
def mp1_session(emu_lib):
    """get(p1_async) -> (engine, records per stream) of the two captures, run once per engine form and shared by the tests of this module
    (the feeds only read the rings); the engines are closed when the module is done"""
    made = {}

    def get(p1_async):
        if p1_async not in made:
            E = _engine(emu_lib, _mp1_caps(), p1_async)
            made[p1_async] = (E, _run(E, _mp1_caps()))
        return made[p1_async]
    yield get
    for E, _ in made.values():
        E.close()


@pytest.mark.parametrize("p1_async", [False, True])
def test_native_feed_equals_python_loop_and_reference(mp1_session, reflib, p1_async):
    caps, exp = _mp1_caps(), _mp1_reference(reflib)
    E, recs = mp1_session(p1_async)
    H = eng.HdcConsumer(2, lib=E.lib)
    n = eng.feed_hdc_batch(E, H, [0, 1], recs)
    assert n == len(H.events) == len(exp[0]) + len(exp[1])
    assert [s for s, *_ in H.events] == [0] * len(exp[0]) + [1] * len(exp[1])           # all of stream_ids[0] first
    P = eng.HdcConsumer(2, lib=E.lib)
    for k in range(2):
        eng.feed_hdc(E, P, k, recs[k])
    for k in range(2):
        assert _events(H, k) == _events(P, k) == exp[k], (k, len(_events(H, k)), len(exp[k]))
    # the order of the list is the caller's: stream 1 first
    R = eng.HdcConsumer(2, lib=E.lib)
    eng.feed_hdc_batch(E, R, [1, 0], [recs[1], recs[0]])
    assert [s for s, *_ in R.events] == [1] * len(exp[1]) + [0] * len(exp[0])
    assert _events(R, 0) == exp[0] and _events(R, 1) == exp[1]
    for c in (H, P, R):
        c.close()


@pytest.mark.parametrize("piece", [3, 1])
def test_records_in_pieces(mp1_session, reflib, piece):
    caps, exp = _mp1_caps(), _mp1_reference(reflib)
    E, recs = mp1_session(True)
    H = eng.HdcConsumer(2, lib=E.lib)
    calls = 0
    for pos in range(0, max(len(r) for r in recs), piece):
        eng.feed_hdc_batch(E, H, [0, 1], [r[pos:pos + piece] for r in recs])       # (the shorter stream's slices run empty: counts of 0)
        calls += 1
    assert calls >= 32 // piece
    for k in range(2):
        assert _events(H, k) == exp[k], (k, piece)
    H.close()


def test_targets_remap_streams(mp1_session, reflib):
    caps, exp = _mp1_caps(), _mp1_reference(reflib)
    E, recs = mp1_session(True)
    H = eng.HdcConsumer(2, lib=E.lib)
    eng.feed_hdc_batch(E, H, [0, 1], recs, targets=[1, 0])
    assert [s for s, *_ in H.events] == [1] * len(exp[0]) + [0] * len(exp[1])       # delivery order follows stream_ids, the callback names the target
    assert _events(H, 1) == exp[0] and _events(H, 0) == exp[1]
    H.close()


@pytest.mark.parametrize("name", ["fm_mp11_cs16", "fm_mp2_cu8"])
def test_extended_service_modes(emu_lib, reflib, captures, name):
    """P3 (MP2) and P3 + P4 (MP11) frames go through the same feed: lc 1 / 2, the PX ring slot from `sis`"""
    cap = captures(name)
    exp = _reference_hdc(reflib, cap.iq)
    assert len(exp) >= 32
    E = _engine(emu_lib, [cap], True)
    recs = _run(E, [cap])
    fl = recs[0]["flags"]
    assert np.any(fl & eng.REC_P3) and (name != "fm_mp11_cs16" or np.any(fl & eng.REC_P4))
    H = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc_batch(E, H, [0], recs)
    P = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc(E, P, 0, recs[0])
    assert _events(H, 0) == _events(P, 0) == exp, (len(_events(H, 0)), len(exp))
    H.close()
    P.close()
    E.close()


@pytest.mark.parametrize("n_frames, n_packets", [(9, 4), (12, 16)])
def test_am(emu_lib, reflib, n_frames, n_packets):
    """hybrid MA1 (the capture of check_l2_index_end_to_end's AM case).  No existing test runs the consumer on AM; 9 L1 frames is the
    smallest length at which the reference delivers HDC packets on this capture (observed: none at 6, 7, 8; 4 at 9; 8 at 10; 16 at 12)."""
    from nrsc5_amd import synth_am
    cap = synth_am.am_ma1_capture(n_frames, seed=31, cfo_hz=2.0, offset=300)
    exp = _reference_hdc(reflib, cap.iq, mode=ref.MODE_AM)
    assert len(exp) == n_packets and all(c > 0 for _, c, _, _ in exp)
    E = _engine(emu_lib, [cap], False, am=True)
    recs = _run(E, [cap], chunk=32768)
    H = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc_batch(E, H, [0], recs, mode=eng.MODE_AM)
    P = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc(E, P, 0, recs[0], mode=eng.MODE_AM)
    assert _events(H, 0) == _events(P, 0) == exp, (len(_events(H, 0)), len(exp))
    H.close()
    P.close()
    E.close()


N_BLOCKS = 96


def test_false_lock_on_the_batch_path(emu_lib, reflib):
    """FALSE_LOCK_CASES[0] (the reference algorithm locks falsely first, loses sync on the first P1 frame's header and re-acquires)
    as a batch session in appends of about 3 blocks, window pipeline + on-device L2 feedback with verdicts 3 windows late, fed after
    every append: the whole event list must be the reference's.  The consumer is still empty when this loss arrives (the false lock ends
    on the header of the first P1 frame), so this case says nothing about what a loss does to packets the consumer holds:
    test_loss_of_sync_with_packets_held does."""
    sd, cfo, off = ec.FALSE_LOCK_CASES[0]
    cap = synth.fm_mp1_capture(0, seed=sd, cfo_hz=cfo, offset=off, snr_db=20, n_blocks=N_BLOCKS)
    iq = cap.iq[:cap.iq.size - cap.iq.size % 4]
    exp = _reference_hdc(reflib, iq)
    assert len(exp) >= 32
    E = eng.Engine(max_streams=1, q15_capacity=iq.size // 4 + 1024, record_capacity=1024, p1_slots=16, p1_async=True, l2_feedback=True, lib_path=emu_lib)
    E.tune(eng.TUNE_VERDICT_LAG, 3)
    dev = ec._to_device(E, iq)
    H = eng.HdcConsumer(1, lib=E.lib)
    lost_at, fed = None, 0
    try:
        for pos in range(0, iq.size, 3 * tc.BLOCK * 4):
            E.batch_append_cu8(dev + pos, 0, [min(3 * tc.BLOCK * 4, iq.size - pos)])
            E.batch_process(1)
            r = E.drain(0)
            if np.any(r["flags"] & eng.REC_LOST_SYNC) and lost_at is None:
                lost_at = len(H.events)
            eng.feed_hdc_batch(E, H, [0], [r])
            fed += len(r)
    finally:
        ec._free_device(E, dev)
        E.close()
    assert lost_at is not None, "the scene does not lose sync"
    print("packets before the loss of sync:", lost_at, "in all:", len(H.events))
    got = _events(H, 0)
    assert len(got) >= 32 and got == exp, (lost_at, len(got), len(exp))
    H.close()


LATENCY = 4          # the PDU header's latency field of the scene below: the reader of the elastic buffer runs 2 * LATENCY packets behind the writer


def _with_latency(make_pdu):
    """synth.make_audio_pdu with the header's latency field set (frame.c:605: output_offset = pdu_seq * avg - 2 * latency) and the
    header's RS parity redone"""
    def make(*args, **kw):
        pdu, packets = make_pdu(*args, **kw)
        pdu = bytearray(pdu)
        pdu[10] |= (LATENCY & 3) << 6
        pdu[11] |= LATENCY >> 2
        par = synth._GF.rs_parity([0] * 159 + [pdu[254 - k] for k in range(159, 247)])
        for k in range(8):
            pdu[7 - k] = par[k]
        return bytes(pdu), packets
    return make


def test_loss_of_sync_with_packets_held(emu_lib, reflib, monkeypatch):
    """What a loss of sync does to the consumer, decided against the reference's events.  Two 3-frame MP1 captures back to back: the
    stream loses sync on the first P1 frame behind the seam and re-acquires.  With the generator's latency of 0 a P1 frame's 32
    packets are gone exactly when the next P1 frame is due -- the only place where an FM stream can lose sync -- so the consumer would
    be empty at the loss; with a latency of 4 it holds 8.  The reference (input_set_sync_state only reports; output_advance stands
    in front of the sync-state test, acquire.c:108) delivers those 8 in the 4 blocks behind the loss, while the stream re-acquires
    and before any new frame arrives.  So must the feed; a consumer that is reset on the loss does not."""
    monkeypatch.setattr(synth, "make_audio_pdu", _with_latency(synth.make_audio_pdu))
    caps = [synth.fm_mp1_capture(3, seed=61 + k, cfo_hz=c, offset=o, snr_db=22) for k, (c, o) in enumerate([(25.0, 400), (-310.0, 3100)])]
    monkeypatch.undo()
    iq = np.concatenate([c.iq for c in caps])
    iq = iq[:iq.size - iq.size % 4]
    log, _, _ = reflib.run(iq, taps=ref.TAP_HDC)
    exp = [(v["program"], v["count"], v["flags"], bytes(v["data"])) for k, v in log if k == "hdc"]
    kinds = [k for k, _ in log if k in ("hdc", "lost_sync")]
    assert kinds.count("lost_sync") == 1
    ref_before = kinds.index("lost_sync")                                            # HDC events the reference fired before its LOST_SYNC
    assert ref_before >= 32 and len(exp) >= ref_before + 2 * LATENCY + 16            # packets before, the held ones, and new ones after re-acquisition
    E = eng.Engine(max_streams=1, q15_capacity=iq.size // 4 + 200000, record_capacity=1024, p1_slots=16, lib_path=emu_lib, p1_async=True, l2_feedback=True)
    common.run_engine_streaming(E, 0, iq)
    recs = E.drain(0)
    lost = np.nonzero(recs["flags"] & eng.REC_LOST_SYNC)[0]
    assert lost.size == 1
    i = int(lost[0])
    behind = recs[i + 1:i + 1 + LATENCY]
    assert not np.any(behind["flags"] & (eng.REC_P1 | eng.REC_P3 | eng.REC_P4))      # no frame arrives in these blocks: what comes out was held
    assert behind["state_after"][0] != eng.SYNC_FINE
    H = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc_batch(E, H, [0], [recs[:i + 1]])
    lost_at = len(H.events)
    assert lost_at == ref_before > 0
    eng.feed_hdc_batch(E, H, [0], [behind])
    assert len(H.events) == lost_at + 2 * LATENCY                                    # the packets held at the loss keep coming, 2 per block
    eng.feed_hdc_batch(E, H, [0], [recs[i + 1 + LATENCY:]])
    assert _events(H, 0) == exp, (lost_at, len(H.events), len(exp))
    # one call over the whole session gives the same
    W = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc_batch(E, W, [0], [recs])
    assert _events(W, 0) == exp
    # the scene tells the two behaviours apart: an output_reset at the loss loses the held packets
    M = eng.HdcConsumer(1, lib=E.lib)
    eng.feed_hdc_batch(E, M, [0], [recs[:i + 1]])
    M.reset(0)
    eng.feed_hdc_batch(E, M, [0], [recs[i + 1:]])
    assert _events(M, 0) == exp[:lost_at] + exp[lost_at + 2 * LATENCY:]
    for c in (H, W, M):
        c.close()
    E.close()


def test_edges(emu_lib, reflib):
    caps = _mp1_caps()[:1]
    E = _engine(emu_lib, caps, False)
    recs = _run(E, caps)[0]
    H = eng.HdcConsumer(2, lib=E.lib)
    eng.feed_hdc_batch(E, H, [0], [recs[:40]])                                       # some state in the consumer
    events, held = list(H.events), H.host_bytes()
    assert len(events) > 0
    lib = H.lib
    rest = np.ascontiguousarray(recs[40:])

    def feed(ids, ptr, count, mode=eng.MODE_FM, targets=None):
        a = np.array(ids, dtype=np.int32)
        t = None if targets is None else np.array(targets, dtype=np.int32)
        ptrs = (ctypes.c_void_p * 1)(ptr)
        counts = np.array([count], dtype=np.int32)
        return lib.nrsc5hip_hdc_feed(H._h, E._h, len(ids), a.ctypes.data, None if t is None else t.ctypes.data, ptrs, counts.ctypes.data, mode, H._cb, None)

    p = rest.ctypes.data
    for rc in (feed([1], p, len(rest)),                       # the engine has one stream
               feed([-1], p, len(rest)),
               feed([0], p, len(rest), targets=[2]),          # the consumer has two
               feed([0], p, len(rest), targets=[-1]),
               feed([0], None, len(rest)),                    # null records with a count
               feed([0], p, -1),
               feed([0], p, len(rest), mode=2)):
        assert rc == eng.EINVAL
        assert H.events == events and H.host_bytes() == held
    bad = rest.copy()
    bad["p1_slot"] = 99                                       # a slot the engine does not have: refused by the index, before the consumer
    assert np.any(bad["flags"] & eng.REC_P1)
    assert feed([0], bad.ctypes.data, len(bad)) == eng.EINVAL and H.events == events and H.host_bytes() == held
    # nothing to do is not an error
    assert lib.nrsc5hip_hdc_feed(H._h, E._h, 0, None, None, None, None, eng.MODE_FM, H._cb, None) == 0
    assert feed([0], p, 0) == 0 and feed([0], None, 0) == 0
    assert eng.feed_hdc_batch(E, H, [], []) == 0 and eng.feed_hdc_batch(E, H, [0], [rest[:0]]) == 0
    assert H.events == events
    # ... and the session goes on where it was
    eng.feed_hdc_batch(E, H, [0], [rest])
    assert _events(H, 0) == _mp1_reference(reflib)[0]
    H.close()
    E.close()
