"""GPU: nrsc5hip_batch_trim on the MI355X -- the checks of tests/test_trim_cpu.py through the real library on longer scenes and deeper
verdict lags, a WidebandReceiver session three times its FIFO against a receiver that holds everything and against the unmodified
reference, and the command line fed from a pipe."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth
from tests import engine_checks as ec, trim_checks as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 3 * tc.BLOCK
N_BLOCKS = 160
_cache = {}


def _fm_streams():
    """the captures of FALSE_LOCK_CASES, lengthened from N_BLOCKS until a third of each is at least the header's minimum capacity"""
    if "fm" not in _cache:
        n_blocks = max(N_BLOCKS, -(-tc.session_length(tc.min_capacity(CHUNK)) // tc.BLOCK) + 1)
        caps = [synth.fm_mp1_capture(0, seed=sd, cfo_hz=c, offset=o, snr_db=20, n_blocks=n_blocks) for sd, c, o in ec.FALSE_LOCK_CASES]
        _cache["fm"] = [c.iq[:c.iq.size - c.iq.size % 4] for c in caps]
    return _cache["fm"]


@pytest.mark.parametrize("lag", [0, 3, 6])
def test_gpu_trim_is_invisible(hip_lib, lag):
    a, b = tc.check_trim_is_invisible(hip_lib, _fm_streams(), "cu8", CHUNK, lag)
    assert sum(1 for k in range(3) for kk, _ in b.logs[k] if kk == "lost_sync") >= 2
    assert all(np.all(r <= tc.BOUND) for r in b.retained)
    assert b.retained[-1][2] <= tc.BOUND // 2, b.retained[-1]          # the clean stream (FALSE_LOCK_CASES[2])
    print("trims", len(b.retained), "largest retained", int(max(r.max() for r in b.retained)))


def test_gpu_trim_is_invisible_cs16(hip_lib, captures):
    iq = np.ascontiguousarray(captures("fm_cs16_cfo60").iq, dtype=np.int16)
    stream = tc.tile_to(iq, 2 * tc.session_length(tc.min_capacity(CHUNK)), 2)
    tc.check_trim_is_invisible(hip_lib, [stream], "cs16", CHUNK, lag=3)


def test_gpu_trim_is_invisible_am(hip_lib):
    from nrsc5_amd import synth_am
    kws = [dict(n_frames=16, seed=9, cfo_hz=2.0, offset=500, burst=(8.3, 0.5, 40.0)),
           dict(n_frames=16, seed=10, cfo_hz=-3.0, offset=900, burst=(9.6, 0.3, 40.0)),
           dict(n_frames=12, seed=11, cfo_hz=1.0, offset=100)]
    chunk = 3 * tc.BLOCK_AM
    need = 2 * tc.session_length(tc.min_capacity(chunk, am=True))
    streams = [tc.tile_to(np.ascontiguousarray(synth_am.am_ma1_capture(**kw).iq, dtype=np.int16), need, 4) for kw in kws]
    a, b = tc.check_trim_is_invisible(hip_lib, streams, "cs16", chunk, lag=3, am=True)
    assert sum(1 for k in range(3) for kk, _ in b.logs[k] if kk == "lost_sync") >= 2


def test_gpu_overlapping_move_fm(hip_lib):
    """trims while most of the slab is unread: k_trim_move_overlap, shift beyond one LDS pass"""
    streams = []
    for sd, nb in ((34, 12), (35, 11), (36, 24)):
        c = synth.fm_mp1_capture(0, seed=sd, cfo_hz=50.0, offset=100, snr_db=18, n_blocks=nb)
        streams.append(c.iq[:c.iq.size - c.iq.size % 4])
    tc.check_overlapping_move(hip_lib, streams, "cu8", steps=2, lag=3)


def test_gpu_overlapping_move_am(hip_lib):
    """... and with a shift below one LDS pass (AM blocks: ~8.6 k samples)"""
    from nrsc5_amd import synth_am
    iq = np.ascontiguousarray(synth_am.am_ma1_capture(n_frames=3, seed=12, cfo_hz=1.0, offset=300).iq, dtype=np.int16)
    tc.check_overlapping_move(hip_lib, [iq[:iq.size - iq.size % 4]], "cs16", steps=1, am=True, want_inside_stage=True)


# ---- WidebandReceiver: a session of three times the FIFO ---------------------------------------------------------------------------
RATE, FMT, OFFS, LEVELS = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
PUSH = 1_000_003                                                       # samples per push


def _band_scene():
    """a 2.4 MS/s cu8 scene of 3 stations, repeated until every station is pushed at least 3 times the small receiver's capacity (the
    header's minimum rounded up to the push); the seam between two copies is a legitimate loss of sync"""
    if "band" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)))
              for k, (o, a) in enumerate(zip(OFFS, LEVELS))]
        cap = sw.capture(st, RATE, FMT, n_frames=2, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        m = int(PUSH * 744187.5 / RATE) + 2                            # outputs of one push at most
        capacity = -(-(tc.BOUND + m) // m) * m
        n_one = cap.raw.numel() // 2
        need = int(3 * capacity * RATE / 744187.5) + PUSH
        raw = cap.raw.repeat(-(-need // n_one))
        torch.cuda.synchronize()
        _cache["band"] = (raw, capacity)
    return _cache["band"]


def _receive(raw, capacity, hip_lib):
    from nrsc5_amd import wideband
    rx = wideband.WidebandReceiver(RATE, FMT, OFFS, q15_capacity=capacity, lib_path=hip_lib)
    n = raw.numel() // 2
    for p in range(0, n, PUSH):
        rx.push(raw[2 * p:2 * min(n, p + PUSH)])
    return rx


def _same_logs(a, b):
    if len(a) != len(b):
        return False
    for (ka, va), (kb, vb) in zip(a, b):
        if ka != kb or va.keys() != vb.keys():
            return False
        for key in va:
            x, y = va[key], vb[key]
            if isinstance(x, np.ndarray):
                if x.tobytes() != y.tobytes():
                    return False
            elif isinstance(x, float):
                if np.float64(x).tobytes() != np.float64(y).tobytes():
                    return False
            elif x != y:
                return False
    return True


def test_gpu_wideband_session_of_three_times_the_fifo(hip_lib, reflib):
    import argparse
    import bench
    from tests.test_gpu_batch256 import HARD_CLASSES
    raw, capacity = _band_scene()
    n = raw.numel() // 2
    S = len(OFFS)
    rx = _receive(raw, capacity, hip_lib)
    pushed = int(n * 744187.5 / RATE)
    assert pushed >= 3 * capacity, (pushed, capacity)
    assert rx.trims >= 2 and rx.max_retained <= tc.BOUND, (rx.trims, rx.max_retained)
    assert 4 * rx.trims <= rx.pushes, (rx.trims, rx.pushes)            # amortised: most pushes copy nothing
    print("pushes", rx.pushes, "trims", rx.trims, "largest retained", rx.max_retained, "capacity", capacity)
    big = _receive(raw, pushed + 4 * 71280, hip_lib)
    assert big.trims == 0
    for s in range(S):
        assert len(rx.station_records(s)) > 0
        assert rx.station_records(s).tobytes() == big.station_records(s).tobytes(), s
        assert _same_logs(rx.logs[s], big.logs[s]), s
        _cache.setdefault("syncs", {})[s] = sum(1 for k, _ in rx.logs[s] if k == "sync")
    big.close()
    # the unmodified reference on the very cs16 bytes the engine decoded (a second channelizer: byte identity across chunkings is guaranteed)
    ch = eng.Channelizer(RATE, eng.IQ_FORMATS[FMT], OFFS, lib_path=hip_lib)
    step = 8 * PUSH
    total = ch.outputs_for(n)                                          # what the receiver's channelizer delivered for the same n samples
    y = np.concatenate([ch.process_tensor(raw[2 * p:2 * min(n, p + step)]).cpu().numpy() for p in range(0, n, step)], axis=1)
    ch.close()
    assert y.shape[1] == total and 0 <= pushed - total <= 16, (y.shape[1], total, pushed)     # (the filter's latency: a few outputs short of n * 744187.5 / rate)
    recs = [rx.station_records(s) for s in range(S)]
    counts = np.array([len(r) for r in recs])
    R = np.zeros((S, max(counts)), dtype=eng.RECORD_DTYPE)
    for s in range(S):
        R[s, :counts[s]] = recs[s]
    W = argparse.Namespace()
    W.eng, W.name, W.my_streams, W.checkable = eng, "wideband-trim", list(range(S)), list(range(S))
    W.args = argparse.Namespace(oracle_streams=-1, oracle_lost_max=S, parity_processes=S)
    W.stream_iq = lambda k: np.ascontiguousarray(y[k].reshape(-1))
    W.impaired = lambda k: False
    n_fail0 = len(bench.FAILURES)
    out = bench.reference_equality(W, R, counts, [None] * S, lambda k, r, fr: rx.logs[k], am=False)
    del bench.FAILURES[n_fail0:]
    print({k: v for k, v in out.items() if k not in ("compared", "checker")})
    assert out["kind"] == "reference" and out["streams_compared"] == S
    classes = out["streams_failing_by_class"]
    assert not any(c in classes for c in HARD_CLASSES), (classes, out["first_diffs"])
    assert S - out["streams_equal_under_the_strict_rule"] <= 1, (classes, out["first_diffs"])
    for s in range(S):
        assert any(k == "sync" for k, _ in rx.logs[s]), s
    rx.close()


def test_gpu_cli_reads_a_pipe_of_any_length(hip_lib):
    """the same bytes through `python -m nrsc5_amd.wideband -` in a fresh child process, default capacity and chunk: the session is longer than
    the FIFO, which the command line no longer sizes from a file length"""
    raw, _ = _band_scene()
    data = raw.cpu().numpy().tobytes()
    assert len(data) // 2 * 744187.5 / RATE > 1.5 * (1 << 24)
    r = subprocess.run([sys.executable, "-m", "nrsc5_amd.wideband", "-", "--format", FMT, "--rate", str(RATE),
                        "--offsets", ",".join(str(o) for o in OFFS)], cwd=ROOT, input=data, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    for s, o in enumerate(OFFS):
        syncs = [l for l in lines if l.startswith(f"station {s} ({o / 1e3:+.1f} kHz): SYNC ")]
        assert len(syncs) >= 1, (s, lines[:20])
        if "syncs" in _cache:                                          # one SYNC line per lock of the station: as many as the in-process receiver logged
            assert len(syncs) == _cache["syncs"][s], (s, len(syncs), _cache["syncs"][s])


def test_gpu_cli_stdin_needs_offsets():
    r = subprocess.run([sys.executable, "-m", "nrsc5_amd.wideband", "-", "--format", FMT, "--rate", str(RATE)], cwd=ROOT,
                       input=b"", capture_output=True, timeout=300)
    assert r.returncode != 0 and b"usage:" in r.stderr and b"--offsets" in r.stderr, r.stderr[-500:]
