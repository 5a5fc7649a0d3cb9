"""`-m "not gpu"`: nrsc5hip_batch_trim on the CPU-emulated twin.  A batch session (window pipeline + on-device L2 feedback, false locks,
rewinds, re-acquisition) through an engine whose FIFO is the header's minimum -- NRSC5HIP_TRIM_RETAIN_MAX + the largest append, at
most a third of the session -- and trimmed whenever the next append would not fit must deliver, byte for byte, what an engine that
holds the whole session delivers; the retained span obeys the stated bound after every trim; the edges of the call."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth
from tests import common, engine_checks as ec, trim_checks as tc

CHUNK = 3 * tc.BLOCK                          # about 3 blocks per append
N_BLOCKS = 96
_cache = {}


def _fm_scene():
    """the captures of FALSE_LOCK_CASES (two false locks, rewinds, re-acquisition), lengthened from N_BLOCKS until a third of each is at
    least the header's minimum capacity for CHUNK-sized appends"""
    if "fm" not in _cache:
        n_blocks = max(N_BLOCKS, -(-tc.session_length(tc.min_capacity(CHUNK)) // tc.BLOCK) + 1)
        caps = [synth.fm_mp1_capture(0, seed=sd, cfo_hz=c, offset=o, snr_db=20, n_blocks=n_blocks) for sd, c, o in ec.FALSE_LOCK_CASES]
        _cache["fm"] = (caps, [c.iq[:c.iq.size - c.iq.size % 4] for c in caps], n_blocks)
    return _cache["fm"]


def _fm_sessions(emu_lib, lag):
    if ("fm", lag) not in _cache:
        _, streams, _ = _fm_scene()
        _cache[("fm", lag)] = tc.check_trim_is_invisible(emu_lib, streams, "cu8", CHUNK, lag)
    return _cache[("fm", lag)]


@pytest.mark.parametrize("lag", [0, 3])
def test_trim_is_invisible(emu_lib, lag):
    a, b = _fm_sessions(emu_lib, lag)
    n_blocks = _fm_scene()[2]
    for k in range(3):
        assert sum(1 for kk, _ in b.logs[k] if kk == "frame") >= n_blocks // 16 - 2
    assert sum(1 for k in range(3) for kk, _ in b.logs[k] if kk == "lost_sync") >= 2      # the scene exercises the replay


def test_trimmed_session_equals_reference(emu_lib, oracle):
    """the trimmed engine's log (verdicts 3 windows late) against the oracle driven by the restated frame_process decision, under the
    rule and the exemptions of engine_checks.check_deferred_feedback_equals_reference"""
    caps, streams, n_blocks = _fm_scene()
    _, b = _fm_sessions(emu_lib, 3)
    lost = 0
    for k, c in enumerate(caps):
        ol, _, _ = oracle.run(streams[k], p1_hook=oracle.l2_hook())
        log = b.logs[k]
        diffs = common.compare_logs(common.strip_states(ol), common.strip_states(log))
        kept = [x for x in common.strip_states(ol) if x[0] not in ("hdc", "soft", "vit", "amsym", "pxsoft")]
        bad = {i for i, (kk, v) in enumerate(kept) if kk == "ber" and v["cber"] > 0.02}
        diffs = [d for d in diffs if not any(d.startswith(f"#{i} ber") or d.startswith(f"#{i + 1} frame") for i in bad)]
        assert not diffs, (k, diffs[:10])
        lost += sum(1 for kk, _ in ol if kk == "lost_sync")
        truth = {np.packbits(f, bitorder="little").tobytes() for f in c.p1_frames}
        good = sum(1 for kk, v in log if kk == "frame" and np.packbits(v["bits"], bitorder="little").tobytes() in truth)
        assert good >= n_blocks // 16 - 2, (k, good)
    assert lost >= 2, "captures do not exercise the feedback"


def test_trim_is_invisible_cs16(emu_lib, captures):
    iq = np.ascontiguousarray(captures("fm_cs16_cfo60").iq, dtype=np.int16)
    stream = tc.tile_to(iq, 2 * tc.session_length(tc.min_capacity(CHUNK)), 2)
    tc.check_trim_is_invisible(emu_lib, [stream], "cs16", CHUNK, lag=3)


def test_trim_is_invisible_am(emu_lib):
    """AM streams with failing PDU headers (the scene of check_am_deferred_feedback_equals_reference): k_rollback_am's checkpoints"""
    from nrsc5_amd import synth_am
    kws = [dict(n_frames=16, seed=9, cfo_hz=2.0, offset=500, burst=(8.3, 0.5, 40.0)),
           dict(n_frames=16, seed=10, cfo_hz=-3.0, offset=900, burst=(9.6, 0.3, 40.0)),
           dict(n_frames=12, seed=11, cfo_hz=1.0, offset=100)]
    chunk = 3 * tc.BLOCK_AM
    need = 2 * tc.session_length(tc.min_capacity(chunk, am=True))
    streams = [tc.tile_to(np.ascontiguousarray(synth_am.am_ma1_capture(**kw).iq, dtype=np.int16), need, 4) for kw in kws]
    a, b = tc.check_trim_is_invisible(emu_lib, streams, "cs16", chunk, lag=3, am=True)
    assert sum(1 for k in range(3) for kk, _ in b.logs[k] if kk == "lost_sync") >= 2


def test_retained_span_obeys_the_bound(emu_lib):
    """retained <= NRSC5HIP_TRIM_RETAIN_MAX after every trim is asserted inside every session (trim_checks.run_session); on a clean
    stream that stays FINE (FALSE_LOCK_CASES[2]) the last trim leaves far less: at most half the bound, or the floor rule keeps
    checkpoints it need not keep"""
    for lag in (0, 3):
        _, b = _fm_sessions(emu_lib, lag)
        assert all(np.all(r <= tc.BOUND) for r in b.retained)
        assert b.retained[-1][2] <= tc.BOUND // 2, b.retained[-1]


def test_overlapping_move_fm(emu_lib):
    """trims with 2 blocks consumed and up to 10 unread: shift ~138 k samples < live span, beyond one LDS pass"""
    streams = [_small_capture(seed=34, n_blocks=12), _small_capture(seed=35, n_blocks=11)]
    tc.check_overlapping_move(emu_lib, streams, "cu8", steps=2, lag=3)


def test_overlapping_move_am(emu_lib):
    """AM blocks are ~8.6 k samples: a trim after every block shifts by less than one LDS pass (12 288), so the source and the destination
    of a single pass overlap"""
    from nrsc5_amd import synth_am
    iq = np.ascontiguousarray(synth_am.am_ma1_capture(n_frames=3, seed=12, cfo_hz=1.0, offset=300).iq, dtype=np.int16)
    tc.check_overlapping_move(emu_lib, [iq[:iq.size - iq.size % 4]], "cs16", steps=1, am=True, want_inside_stage=True)


def _small_capture(seed=31, n_blocks=6):
    cap = synth.fm_mp1_capture(0, seed=seed, cfo_hz=50.0, offset=100, snr_db=18, n_blocks=n_blocks)
    return cap.iq[:cap.iq.size - cap.iq.size % 4]


def test_trim_edges(emu_lib):
    iq = _small_capture()
    E = eng.Engine(max_streams=2, q15_capacity=iq.size // 4 + 71280, record_capacity=256, p1_slots=4, p1_async=True, l2_feedback=True, lib_path=emu_lib)
    assert E.batch_trim(2).tolist() == [0, 0]                                  # fresh streams: nothing to give back
    for bad in ([2], [-1], [0, 7]):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            E.batch_trim(len(bad), stream_ids=bad)
        assert ("error %d:" % eng.EINVAL) in str(ei.value)
    with pytest.raises(eng.Nrsc5HipError):
        E.batch_trim(3)                                                        # more streams than the engine has
    dev = ec._to_device(E, iq)
    E.batch_append_cu8(dev, 0, [iq.size], stream_ids=[1])
    assert E.batch_trim(1, stream_ids=[1]).tolist() == [iq.size // 4]          # nothing processed yet: everything may still be read
    E.batch_process(1, stream_ids=[1])
    first = E.batch_trim(2)
    assert first[0] == 0 and 0 < first[1] < 71280, first                       # the unread tail: less than one window
    assert E.batch_trim(2).tolist() == first.tolist()                          # a trim directly behind a trim retains the same
    with pytest.raises(eng.Nrsc5HipError) as ei:
        E.batch_trim(2, stream_ids=[1, 1])                                     # two grid rows would move the same span
    assert ("error %d:" % eng.EINVAL) in str(ei.value) and "twice" in str(ei.value)
    n_recs = len(E.drain(1))
    assert n_recs >= 5
    # the space is really back: the whole capture fits again, which it would not behind the untrimmed samples
    E.batch_append_cu8(dev, 0, [iq.size], stream_ids=[1])
    with pytest.raises(eng.Nrsc5HipError) as ei:
        E.batch_append_cu8(dev, 0, [iq.size], stream_ids=[1])                  # appends never trim by themselves
    assert tc.is_overflow(ei.value) and "retained" in str(ei.value)
    ec._free_device(E, dev)
    E.close()


def test_trim_leaves_a_zero_copy_stream_alone(emu_lib):
    iq = _small_capture(seed=32, n_blocks=20)
    logs = []
    for trim in (False, True):
        E = eng.Engine(max_streams=1, q15_capacity=2 * 71280, record_capacity=256, p1_slots=4, p1_async=True, l2_feedback=True, batch_zero_copy=True, lib_path=emu_lib)
        dev = ec._to_device(E, iq)
        E.batch_append_cu8(dev, 0, [iq.size])
        if trim:
            assert E.batch_trim(1).tolist() == [0]
        E.batch_process(1, max_steps=7)
        if trim:
            assert E.batch_trim(1).tolist() == [0]
        E.batch_process(1)
        if trim:
            assert E.batch_trim(1).tolist() == [0]
        logs.append(E.drain(0).tobytes())
        ec._free_device(E, dev)
        E.close()
    assert len(logs[0]) >= 19 * eng.RECORD_DTYPE.itemsize and logs[0] == logs[1]


def test_trim_does_not_disturb_the_streaming_seam_of_another_stream(emu_lib, captures):
    """stream 0: the streaming seam with a FIFO so small that it compacts many times (check_small_fifo_compaction), against the golden
    log; between its pushes stream 1 of the same engine is fed through the batch path and trimmed"""
    name = "fm_cu8_cfo-2400"
    g = ec.golden(name)
    cap = captures(name)
    chunk = 4 * 9000
    other = _small_capture(seed=33, n_blocks=8)
    E = eng.Engine(max_streams=2, q15_capacity=2 * 71280 + chunk // 4, lib_path=emu_lib)
    dev = ec._to_device(E, other)
    iq = cap.iq[:cap.iq.size - cap.iq.size % 4]
    pos1, trims, n1 = 0, 0, 0
    for pos in range(0, iq.size, chunk):
        E.push_cu8(0, iq[pos:pos + chunk])
        if pos1 < other.size:
            nb = min(chunk, other.size - pos1)
            E.batch_trim(1, stream_ids=[1]); trims += 1
            E.batch_append_cu8(dev + pos1, 0, [nb], stream_ids=[1])
            E.batch_process(1, stream_ids=[1])
            n1 += len(E.drain(1))
            pos1 += nb
    log = eng.records_to_log(E, 0, E.drain(0))
    diffs = common.compare_logs(common.arrays_to_log(g), common.strip_states(log))
    assert not diffs, diffs[:10]
    assert trims >= 8 and n1 >= 6, (trims, n1)                                 # stream 1 ran through a FIFO a fifth of its capture
    ec._free_device(E, dev)
    E.close()


def test_trim_of_a_stream_the_streaming_seam_feeds(emu_lib, captures):
    """a stream driven by pushes (fast seam, FIFO form: no pinned capture) is trimmed between pushes, with a block step possibly still in
    flight and samples staged on the host: the call settles the seam first, and the stream, read from the device from then on as after
    every batch entry point, still delivers the golden log"""
    name = "fm_cu8_cfo-2400"
    g = ec.golden(name)
    cap = captures(name)
    chunk = 4 * 9000
    iq = cap.iq[:cap.iq.size - cap.iq.size % 4]
    E = eng.Engine(max_streams=1, q15_capacity=4 * 71280, lib_path=emu_lib)
    E.tune(eng.TUNE_HOST_CAPTURE, 0)
    recs, kept = [], []
    for i, pos in enumerate(range(0, iq.size, chunk)):
        E.push_cu8(0, iq[pos:pos + chunk])
        if i >= 40 and i % 5 == 0:
            kept.append(int(E.batch_trim(1)[0]))
            recs.append(E.drain(0))
    recs.append(E.drain(0))
    log = eng.records_to_log(E, 0, np.concatenate(recs))
    diffs = common.compare_logs(common.arrays_to_log(g), common.strip_states(log))
    assert not diffs, diffs[:10]
    assert len(kept) >= 10 and all(0 <= k < 2 * 71280 for k in kept), kept
    E.close()


def test_binding_states_the_header_bound():
    import os
    import re
    text = open(os.path.join(common.ROOT, "include", "nrsc5hip.h")).read()
    m = re.search(r"#define NRSC5HIP_TRIM_RETAIN_MAX\s+\(\(8LL \* 16 \+ 1\) \* 71280\)", text)
    assert m and eng.TRIM_RETAIN_MAX == (8 * 16 + 1) * 71280
    assert re.search(r"#define NRSC5HIP_TRIM_RETAIN_MAX_AM\s+\(\(8LL \* 8 \+ 1\) \* 8910\)", text) and eng.TRIM_RETAIN_MAX_AM == (8 * 8 + 1) * 8910
    assert (1 << 24) >= eng.TRIM_RETAIN_MAX + 7_000_000                         # the receiver's default carries any session at its default push


def test_cli_stdin_needs_offsets():
    """`-` cannot be scanned: without --offsets the command line is an argparse error, before anything touches a device"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "nrsc5_amd.wideband", "-", "--format", "cu8", "--rate", "2400000"], cwd=common.ROOT,
                       input=b"", capture_output=True, timeout=300)
    assert r.returncode != 0 and b"usage:" in r.stderr and b"--offsets" in r.stderr, r.stderr[-500:]
