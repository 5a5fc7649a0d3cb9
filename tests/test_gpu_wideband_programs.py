"""GPU: the wideband receiver delivers every station's audio programs (WidebandReceiver(programs=True), nrsc5hip_hdc_feed,
`python -m nrsc5_amd.wideband --dump-hdc`).  Every comparison is against the NRSC5_EVENT_HDC sequence of the UNMODIFIED reference run
on the very cs16 bytes each station's engine stream decoded (the channelizer's output, copied back): program, flags and payload of
every packet, in order."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from oracle import ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS, N_FRAMES = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8], 3
_cache = {}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _scene(hip_lib, reflib):
    """the 2.4 MS/s cu8 capture of 3 stations of test_gpu_wideband.test_gpu_end_to_end_small_captures, 3 L1 frames long, and the reference's
    HDC events of every station's channelized stream -- computed once, shared by the tests below"""
    if "scene" not in _cache:
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)))
              for k, (o, a) in enumerate(zip(OFFS, LEVELS))]
        cap = sw.capture(st, RATE, FMT, n_frames=N_FRAMES, noise_rms=0.02, seed=3, device=_dev())
        ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
        y = ch.process_tensor(cap.raw).cpu().numpy()
        ch.close()
        exp = []
        for s in range(len(OFFS)):
            log, _, _ = reflib.run(np.ascontiguousarray(y[s].reshape(-1)), taps=ref.TAP_HDC)
            exp.append([(v["program"], v["flags"], bytes(v["data"])) for k, v in log if k == "hdc"])
            assert len(exp[s]) >= 16, (s, len(exp[s]))                # on the reference alone: the scene must carry audio for every station
        _cache["scene"] = (cap, exp)
    return _cache["scene"]


def _receive(cap, chunk, hip_lib, programs=True, q15=None, on_packet=None):
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    if q15 is None:
        q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFS, q15_capacity=q15, lib_path=hip_lib, programs=programs, on_packet=on_packet)
    for p in range(0, n, chunk):
        rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
    return rx


def _plain(cap, hip_lib):
    """the untrimmed programs=True session in pushes of 1 << 20 samples"""
    if "plain" not in _cache:
        seen = []
        rx = _receive(cap, 1 << 20, hip_lib, on_packet=lambda s, p, f, d: seen.append((s, p, f, d)))
        _cache["plain"] = ([list(p) for p in rx.packets], rx.logs, seen)
        rx.close()
    return _cache["plain"]


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_every_station_delivers_the_reference_packets(hip_lib, reflib):
    cap, exp = _scene(hip_lib, reflib)
    packets, logs, seen = _plain(cap, hip_lib)
    for s in range(len(OFFS)):
        assert packets[s] == exp[s], (s, len(packets[s]), len(exp[s]))
    # on_packet saw every packet, in the order of each station's list
    for s in range(len(OFFS)):
        assert [(p, f, d) for (t, p, f, d) in seen if t == s] == packets[s]
    # programs=True changes nothing else: the event logs are those of a receiver without it, which collects no packets
    rx = _receive(cap, 1 << 20, hip_lib, programs=False)
    assert rx.hdc is None and rx.packets == [[] for _ in OFFS]
    for s in range(len(OFFS)):
        _same_logs(rx.logs[s], logs[s])
    rx.close()


def test_gpu_trimmed_session_delivers_the_same_packets(hip_lib, reflib):
    """a receiver of the minimum capacity (eng.TRIM_RETAIN_MAX + the outputs of one push) against one that holds the whole session, and
    both against the reference.  The minimum capacity is 9.2 M outputs per station and the capture has 3.3 M, so nothing would ever be
    trimmed on it: the session here is the capture three times over (as tests/test_gpu_trim.py builds its band scene; the seam between
    two copies is a loss of sync like any other), just longer than the capacity.  The trim moves the sample FIFO only: the ring slots
    the records name stay as they are.  The reference runs on every station's channelized bytes of the WHOLE tiled session, so the
    packets around both seams -- a loss of sync and a re-acquisition each -- are held to its events too."""
    cap, exp = _scene(hip_lib, reflib)
    chunk = 1 << 19
    raw = cap.raw.repeat(3)
    n = raw.numel() // 2
    probe = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
    q15 = eng.TRIM_RETAIN_MAX + probe.outputs_for(chunk) + 1          # (+ 1: the ratio is not an integer, one push in some gives one output more)
    assert probe.outputs_for(n) > q15 + probe.outputs_for(chunk), "the session fits the minimum capacity: nothing would be trimmed"
    y = probe.process_tensor(raw).cpu().numpy()
    probe.close()
    from nrsc5_amd import wideband

    def session(capacity):
        rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFS, q15_capacity=capacity, lib_path=hip_lib, programs=True)
        for p in range(0, n, chunk):
            rx.push(raw[2 * p:2 * min(n, p + chunk)])
        out = ([list(p) for p in rx.packets], rx.trims, [sum(1 for k, _ in log if k == "lost_sync") for log in rx.logs])
        rx.close()
        return out

    small, trims, lost = session(q15)
    assert trims >= 1
    big, none, _ = session(int(n / float(cap.rate) * 744187.5) + 4 * 71280)
    assert none == 0
    for s in range(len(OFFS)):
        log, _, _ = reflib.run(np.ascontiguousarray(y[s].reshape(-1)), taps=ref.TAP_HDC)
        want = [(v["program"], v["flags"], bytes(v["data"])) for k, v in log if k == "hdc"]
        assert sum(1 for k, _ in log if k == "lost_sync") >= 2 and lost[s] >= 2, (s, lost[s])      # both seams
        assert len(want) > 2 * len(exp[s]), (s, len(want), len(exp[s]))                            # packets of every copy
        assert small[s] == want and big[s] == want, (s, len(small[s]), len(big[s]), len(want))


def test_gpu_packets_do_not_depend_on_the_push_size(hip_lib, reflib):
    cap, exp = _scene(hip_lib, reflib)
    packets, _, _ = _plain(cap, hip_lib)                              # pushes of 1 << 20
    rx = _receive(cap, 1 << 18, hip_lib)
    for s in range(len(OFFS)):
        assert rx.packets[s] == packets[s], s
    rx.close()


def _expected_files(exp):
    """{file name: (bytes, packets)} of --dump-hdc from the reference's events: ADTS frames of the packets that carry data"""
    H = eng.HdcConsumer(1)
    files = {}
    for s, events in enumerate(exp):
        for program in sorted({p for p, _, _ in events}):
            frames = [H.adts(d) for p, _, d in events if p == program and len(d) > 0]
            if frames:
                files["station%d_%+d_p%d.aac" % (s, int(round(OFFS[s])), program)] = (b"".join(frames), len(frames))
    H.close()
    return files


def _check_dump(out_dir, stdout, exp):
    want = _expected_files(exp)
    assert len(want) >= len(OFFS)
    assert sorted(os.listdir(out_dir)) == sorted(want)
    lines = [l for l in stdout.splitlines() if ": program " in l]
    assert len(lines) == len(want), stdout
    for name, (data, n) in want.items():
        assert open(os.path.join(out_dir, name), "rb").read() == data, name
        s, program = int(name.split("_")[0][len("station"):]), int(name.rsplit("_p", 1)[1][:-len(".aac")])
        line = "station %d (%+.1f kHz): program %d packets %d bytes %d" % (s, OFFS[s] / 1e3, program, n, len(data))
        assert line in lines, (line, lines)


@pytest.mark.parametrize("source", ["file", "pipe"])
def test_gpu_cli_dump_hdc(hip_lib, reflib, tmp_path, source):
    cap, exp = _scene(hip_lib, reflib)
    f = tmp_path / "band.cu8"
    raw = cap.raw.cpu().numpy()
    raw.tofile(f)
    out = tmp_path / "hdc"
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", "-" if source == "pipe" else str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(1 << 20), "--dump-hdc", str(out)]
    # a fresh child process; the pipe case gets the capture's bytes through its standard input
    r = subprocess.run(cmd, cwd=ROOT, input=raw.tobytes() if source == "pipe" else b"", capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    stdout = r.stdout.decode()
    assert sum(" SYNC " in l for l in stdout.splitlines()) >= len(OFFS)
    _check_dump(str(out), stdout, exp)


def test_gpu_native_feed_on_the_device(hip_lib, reflib):
    """nrsc5hip_hdc_feed over two batch streams of the gfx950 library (window pipeline, on-device L2 feedback) == the Python loop
    eng.feed_hdc == the reference.  The captures are those of engine_checks.check_l2_index_fused at 3 L1 frames: at its 2 the
    reference delivers 32 HDC packets on the first and none on the second, which misses the floor of 32; at 3 it delivers 64 and 32."""
    from nrsc5_amd import synth
    from tests import engine_checks as ec
    caps = [synth.fm_mp1_capture(3, seed=61 + k, cfo_hz=c, offset=o, snr_db=22) for k, (c, o) in enumerate([(25.0, 400), (-310.0, 3100)])]
    streams = [c.iq[:c.iq.size - c.iq.size % 4] for c in caps]
    exp = []
    for iq in streams:
        log, _, _ = reflib.run(iq, taps=ref.TAP_HDC)
        exp.append([(v["program"], v["count"], v["flags"], bytes(v["data"])) for k, v in log if k == "hdc"])
        assert len(exp[-1]) >= 32
    stride = max(s.size for s in streams); stride += (-stride) % 256
    buf = np.zeros((2, stride), dtype=np.uint8)
    for k, s in enumerate(streams):
        buf[k, :s.size] = s
    E = eng.Engine(max_streams=2, q15_capacity=stride // 4 + 1024, record_capacity=1024, p1_slots=16, p1_async=True, l2_feedback=True, lib_path=hip_lib)
    dev = ec._to_device(E, buf)
    H, P = eng.HdcConsumer(2, lib=E.lib), eng.HdcConsumer(2, lib=E.lib)
    try:
        E.batch_append_cu8(dev, stride, [s.size for s in streams])
        E.batch_process(2)
        recs = [E.drain(k) for k in range(2)]
        n = eng.feed_hdc_batch(E, H, [0, 1], recs)
        for k in range(2):
            eng.feed_hdc(E, P, k, recs[k])
    finally:
        ec._free_device(E, dev)
        E.close()
    assert n == len(H.events) == len(exp[0]) + len(exp[1])
    for k in range(2):
        got = [(p, c, f, d) for (s, p, c, f, d) in H.events if s == k]
        assert got == [(p, c, f, d) for (s, p, c, f, d) in P.events if s == k] == exp[k], (k, len(got), len(exp[k]))
    H.close()
    P.close()
