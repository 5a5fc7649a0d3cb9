"""Checks of nrsc5hip_batch_trim shared by tests/test_trim_cpu.py (CPU-emulated twin) and tests/test_gpu_trim.py (the gfx950 library): chunked batch sessions
through an engine whose FIFO holds a fraction of the session, trimmed whenever the next append would not fit, against the same
session through an engine that holds everything and never trims."""
import numpy as np

from nrsc5_amd import engine as eng
from tests import engine_checks as ec

BOUND = eng.TRIM_RETAIN_MAX                 # NRSC5HIP_TRIM_RETAIN_MAX: FM streams
BOUND_AM = eng.TRIM_RETAIN_MAX_AM           # NRSC5HIP_TRIM_RETAIN_MAX_AM
BLOCK = 32 * 2160                           # decimated samples of one FM block
BLOCK_AM = 32 * 270


class Session:
    """per stream: the drained record arrays (concatenated), the ordered log with its frames; and how the trims went"""

    def __init__(self, n):
        self.recs = [[] for _ in range(n)]
        self.logs = [[] for _ in range(n)]
        self.retained = []               # one array per trim
        self.bases_moved = 0

    def records(self, k):
        return np.concatenate(self.recs[k]) if self.recs[k] else np.zeros(0, dtype=eng.RECORD_DTYPE)

    def frames(self, k, kind="frame"):
        return [v["bits"].tobytes() for kk, v in self.logs[k] if kk == kind]


def tile_to(iq: np.ndarray, n_items: int, align: int) -> np.ndarray:
    """the capture repeated until it holds at least n_items items (the seam between two copies is a loss of sync like any other)"""
    reps = -(-n_items // iq.size)
    out = np.tile(iq, reps)
    return out[:out.size - out.size % align]


def min_capacity(chunk_out: int, am: bool = False) -> int:
    """the header's minimum for an endless session: the retention bound + the largest append"""
    return (BOUND_AM if am else BOUND) + chunk_out


def session_length(capacity: int) -> int:
    """decimated samples a capture must have so that the capacity is at most a third of it"""
    return 3 * capacity


def run_session(lib, streams, fmt, capacity, chunk_out, lag=0, trim=True, am=False, tune=(), process=True):
    """streams: one 1-d array per stream (cu8 bytes, or int16 values for "cs16").  Appends chunk_out decimated samples per stream and call,
    processes, drains every stream (records + frames) after each chunk.  trim=True: nrsc5hip_batch_trim whenever the next append would not fit.
    Every retained count is checked against the bound right after its trim (a condition, not a measurement).  process=False: appends only."""
    n = len(streams)
    assert not (am and fmt == "cu8"), "the AM scenes of these checks are cs16"
    per = 4 if fmt == "cu8" else 2                                                   # items per decimated sample
    stride = max(s.size for s in streams); stride += (-stride) % 256
    buf = np.zeros((n, stride), dtype=streams[0].dtype)
    for k, s in enumerate(streams):
        buf[k, :s.size] = s
    E = eng.Engine(max_streams=n, q15_capacity=capacity, record_capacity=1024, p1_slots=16, p1_async=True, l2_feedback=True, am_enable=am, lib_path=lib)
    E.tune(eng.TUNE_VERDICT_LAG, lag)
    for knob, value in tune:
        E.tune(knob, value)
    if am:
        for k in range(n):
            E.set_mode(k, eng.MODE_AM)
    dev = ec._to_device(E, buf)
    out = Session(n)
    bound = BOUND_AM if am else BOUND
    held = np.zeros(n, dtype=np.int64)
    pos = 0
    try:
        while pos < stride:
            counts = [int(max(0, min(chunk_out * per, s.size - pos))) for s in streams]
            counts = [c - c % (4 if fmt == "cu8" else 2) for c in counts]
            if not any(counts):
                break
            add = np.array([c // per for c in counts], dtype=np.int64)
            if trim and np.any(held + add > capacity):
                kept = E.batch_trim(n)
                assert np.all(kept <= held), (kept, held)
                assert np.all(kept <= bound), (kept, bound)
                out.bases_moved += int(np.sum(kept < held))
                out.retained.append(kept.copy())
                held = kept.copy()
            if fmt == "cu8":
                E.batch_append_cu8(dev + pos, stride, counts)
            else:
                E.batch_append_cs16(dev + 2 * pos, stride, counts)
            held += add
            if process:
                E.batch_process(n)
            for k in range(n if process else 0):
                r = E.drain(k)
                if len(r):
                    assert not (r["flags"] & eng.REC_DISCARDED).any()
                    out.recs[k].append(r.copy())
                    out.logs[k] += (eng.am_records_to_log if am else eng.records_to_log)(E, k, r)
            pos += chunk_out * per
    finally:
        ec._free_device(E, dev)
        E.close()
    return out


def assert_sessions_equal(a: Session, b: Session, n: int):
    for k in range(n):
        ra, rb = a.records(k), b.records(k)
        assert len(ra) == len(rb) and len(ra) > 0, (k, len(ra), len(rb))
        assert ra.tobytes() == rb.tobytes(), (k, "records differ", int(np.argmax(ra != rb)))
        assert a.frames(k) == b.frames(k), (k, "P1 / P3 frames differ")
        assert a.frames(k, "pids") == b.frames(k, "pids"), (k, "PIDS frames differ")


def is_overflow(err: Exception) -> bool:
    return isinstance(err, eng.Nrsc5HipError) and ("error %d:" % eng.EOVERFLOW) in str(err)


def check_trim_is_invisible(lib, streams, fmt, chunk_out, lag, am=False, min_trims=3, capacity=None):
    """-> (untrimmed session, trimmed session).  The captures must be at least three times the small engine's capacity."""
    import pytest
    n = len(streams)
    per = 4 if fmt == "cu8" else 2
    cap_b = capacity or min_capacity(chunk_out, am)
    for s in streams:
        assert 3 * cap_b <= s.size // per, ("capture too short for this capacity", s.size // per, cap_b)
    cap_a = max(s.size for s in streams) // per + 1024
    a = run_session(lib, streams, fmt, cap_a, chunk_out, lag, trim=False, am=am)
    assert not a.retained
    b = run_session(lib, streams, fmt, cap_b, chunk_out, lag, trim=True, am=am)
    assert_sessions_equal(a, b, n)
    assert len(b.retained) >= min_trims, len(b.retained)
    assert b.bases_moved >= min_trims * n, (b.bases_moved, len(b.retained))          # every stream gave space back at least that often
    # the capacity really is too small for the session: the same appends without a trim end in EOVERFLOW (whether or not the blocks
    # in between are processed: the appends never give space back by themselves)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        run_session(lib, streams, fmt, cap_b, chunk_out, lag, trim=False, am=am, process=False)
    assert is_overflow(ei.value), str(ei.value)
    assert "retained" in str(ei.value)
    return a, b


STAGE = 12288                               # TRIM_STAGE of k_trim.hip: samples the overlapping move stages through LDS per pass


def run_stepwise(lib, streams, fmt, steps, trim, am=False, lag=0):
    """the whole captures appended at once, then batch_process(max_steps=steps) until nothing is left, every stream drained after each
    call; trim=True: nrsc5hip_batch_trim after every call, while most of the slab is still unread.  -> (Session, [(off, n) per trim and stream])"""
    n = len(streams)
    per = 4 if fmt == "cu8" else 2
    stride = max(s.size for s in streams); stride += (-stride) % 256
    buf = np.zeros((n, stride), dtype=streams[0].dtype)
    for k, s in enumerate(streams):
        buf[k, :s.size] = s
    E = eng.Engine(max_streams=n, q15_capacity=stride // per + 1024, record_capacity=1024, p1_slots=16, p1_async=True, l2_feedback=True, am_enable=am, lib_path=lib)
    E.tune(eng.TUNE_VERDICT_LAG, lag)
    if am:
        for k in range(n):
            E.set_mode(k, eng.MODE_AM)
    dev = ec._to_device(E, buf)
    out, moves = Session(n), []
    counts = [s.size - s.size % (4 if fmt == "cu8" else 2) for s in streams]
    held = np.array([c // per for c in counts], dtype=np.int64)
    try:
        (E.batch_append_cu8 if fmt == "cu8" else E.batch_append_cs16)(dev, stride, counts)
        while True:
            done = E.batch_process(n, max_steps=steps)
            if trim:
                kept = E.batch_trim(n)
                assert np.all(kept <= held), (kept, held)
                moves += [(int(h - k), int(k)) for h, k in zip(held, kept)]
                held = kept.copy()
            for k in range(n):
                r = E.drain(k)
                if len(r):
                    assert not (r["flags"] & eng.REC_DISCARDED).any()
                    out.recs[k].append(r.copy())
                    out.logs[k] += (eng.am_records_to_log if am else eng.records_to_log)(E, k, r)
            if done == 0:
                break
    finally:
        ec._free_device(E, dev)
        E.close()
    return out, moves


def check_overlapping_move(lib, streams, fmt, steps, am=False, lag=0, want_inside_stage=False):
    """A trim while most of the slab is unread moves a span onto itself (shift `off` < live span `n`): k_trim_move_overlap.  The stepwise session with
    such a trim after every call must equal the same session without any, byte for byte; the retained counts prove which moves were of that kind."""
    a, _ = run_stepwise(lib, streams, fmt, steps, trim=False, am=am, lag=lag)
    b, moves = run_stepwise(lib, streams, fmt, steps, trim=True, am=am, lag=lag)
    assert_sessions_equal(a, b, len(streams))
    overlapping = [(off, n) for off, n in moves if 0 < off < n]
    assert len(overlapping) >= 3 * len(streams), moves
    assert any(n > 2 * STAGE for off, n in overlapping), overlapping             # several passes
    if want_inside_stage:
        assert sum(1 for off, n in overlapping if off < STAGE and n > STAGE) >= 3, overlapping     # source and destination of ONE pass overlap
    else:
        assert any(off > STAGE for off, n in overlapping), overlapping
    assert any(0 < n <= off for off, n in moves), moves                           # ... and the session's last moves were disjoint ones
    return a, b, moves
