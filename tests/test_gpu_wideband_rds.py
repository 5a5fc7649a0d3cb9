"""GPU: the wideband receiver decodes RDS / RBDS of every station's analog host (WidebandReceiver(rds=True): FmDemod(rds=True) behind the
channelizer's staged outputs; `python -m nrsc5_amd.wideband --rds`).  The three-station 2.4 MS/s cu8 scene of tests/test_gpu_wideband_analog.py,
one L1 frame long: the first station carries a stereo host with RDS at 4 kHz (PI, name, a 32-character RadioText, one clock group), the second
a mono host with another PI and name, the third no host.  The events of the two hosted stations must equal the float64 model's
(tests/rds_model.py) run on that station's channelized cs16 (Channelizer.process) -- under the asserted proviso (tests/rds_args.analyse) that no
decision of the model on that stream is within reach of float32 rounding -- and what was decoded must be what was sent."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth_fm as sf
from tests import rds_args as ra

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
TEXT = "Now playing: a 32-character text"
CLOCK = (60310, 13, 37, -14)
SENT = [dict(pi=0x3AAB, ps="KEXP-FM ", text=TEXT, clock=CLOCK), dict(pi=0x54A9, ps="WAAB 1  ")]
HOSTS = [dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2, 0.5)], preemph_us=75, rds=dict(groups=sf.rds_groups(pty=5, tp=1, **SENT[0]), dev_hz=4000.0)),
         dict(left=[(2000.0, 0.3)], right=[(2000.0, 0.3)], pilot=None, preemph_us=75, rds=dict(groups=sf.rds_groups(**SENT[1]), dev_hz=4000.0)),
         None]
HOST_DB = 14.0
CHUNK = 1 << 20
_cache = {}


def _scene(hip_lib):
    """-> (capture, per hosted station: the model's run on its channelized stream)"""
    if "scene" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        assert len(TEXT) == 32
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)), host=h, host_db=HOST_DB)
              for k, (o, a, h) in enumerate(zip(OFFS, LEVELS, HOSTS))]
        cap = sw.capture(st, RATE, FMT, n_frames=1, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
        y = ch.process_tensor(cap.raw).cpu().numpy()
        ch.close()
        want = []
        for s in (0, 1):
            ref = ra.analyse(y[s], f"station {s}")             # asserts the margins: if they do not clear the bound, raise the scene's RDS level
            print(f"station {s}: y bound {ref['tol_y']:.3g}, smallest margin: bits {ref['margin_bit']:.3g} x, energies {ref['margin_e']:.3g} x the bound; "
                  f"{ref['stream'].size} bits, {ref['groups'].stats['groups']} groups")
            want.append(ref)
        _cache["scene"] = (cap, want)
    return _cache["scene"]


def _receive(cap, hip_lib, **kw):
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFS, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, **kw)
    events = []
    for p in range(0, n, CHUNK):
        events += rx.push(cap.raw[2 * p:2 * min(n, p + CHUNK)])
    return rx, events


def _rds(hip_lib):
    if "rx" not in _cache:
        cap, _ = _scene(hip_lib)
        rx, events = _receive(cap, hip_lib, analog=True, rds=True)
        _cache["rx"] = ([np.concatenate(a) for a in rx.audio], [list(l) for l in rx.logs], events, rx.rds_info, [rx.fm.rds_stats(s) for s in range(len(OFFS))])
        rx.close()
    return _cache["rx"]


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_events_equal_the_model_and_what_was_sent(hip_lib):
    cap, want = _scene(hip_lib)
    audio, logs, events, info, stats = _rds(hip_lib)
    for s in (0, 1):
        g = want[s]["groups"]
        got = [v for k, v in logs[s] if k == "rds"]
        assert got == [{"kind": e["kind"], **eng.rds_event_fields(e["kind"], e["v"], e["data"])} for e in g.events], (s, got)
        assert got == [v for t, k, v in events if t == s and k == "rds"]           # the events push() returned are the log's
        assert info[s] == g.snapshot() and stats[s] == g.stats, s
        sent = SENT[s]
        assert info[s]["pi"] == sent["pi"] and info[s]["ps"] == sent["ps"].encode() and info[s]["synced"] == 1
        assert [v["ps"] for v in got if v["kind"] == "ps"] == [sent["ps"].rstrip()]
        assert [v["pi"] for v in got if v["kind"] == "pi"] == [sent["pi"]]
        assert want[s]["groups"].stats["groups_dropped"] == 0 and want[s]["groups"].stats["blocks_invalid"] == 0
    assert info[0]["rt"] == (TEXT + "\r").encode().ljust(36)                    # as sent: ended by 0x0D, the ninth segment padded
    assert [v["text"] for k, v in logs[0] if k == "rds" and v["kind"] == "rt"] == [TEXT]
    assert info[0]["clock"] == CLOCK and info[0]["pty"] == 5 and info[0]["tp"] == 1
    assert info[1]["rt"] is None and info[1]["clock"] is None
    assert eng.rds_callsign(info[0]["pi"]) == "KQED" and eng.rds_callsign(info[1]["pi"]) == "WAAB"
    # the station without a host: bits, but no sync and no event
    assert not [v for k, v in logs[2] if k == "rds"] and info[2]["pi"] == -1 and not info[2]["synced"] and stats[2]["bits"] == stats[0]["bits"]


def test_gpu_rds_off_changes_nothing(hip_lib):
    cap, _ = _scene(hip_lib)
    audio, logs, events, info, stats = _rds(hip_lib)
    plain, _ = _receive(cap, hip_lib, analog=True)
    try:
        assert plain.rds_info == [None] * len(OFFS)
        for s in range(len(OFFS)):
            assert np.concatenate(plain.audio[s]).tobytes() == audio[s].tobytes(), s
            assert not any(k == "rds" for k, v in plain.logs[s])
            _same_logs(plain.logs[s], [e for e in logs[s] if e[0] != "rds"])
    finally:
        plain.close()
    only, _ = _receive(cap, hip_lib, rds=True)                   # without analog: the demodulator is there, the audio is not collected
    try:
        assert only.fm is not None and only.audio == [[] for _ in OFFS]
        for s in range(len(OFFS)):
            assert [v for k, v in only.logs[s] if k == "rds"] == [v for k, v in logs[s] if k == "rds"]
            assert not any(k == "analog" for k, v in only.logs[s])
    finally:
        only.close()


def test_gpu_cli_rds_lines(hip_lib, tmp_path):
    cap, _ = _scene(hip_lib)
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(CHUNK), "--rds"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if " RDS " in l]
    assert [l for l in lines if l.startswith("station 0 ")] == ["station 0 (-800.0 kHz): RDS PI 0x3AAB (KQED)",
                                                                f'station 0 (-800.0 kHz): RDS RT "{TEXT}"',
                                                                "station 0 (-800.0 kHz): RDS clock MJD 60310 13:37 UTC-07:00",
                                                                'station 0 (-800.0 kHz): RDS PS "KEXP-FM "'], lines
    assert [l for l in lines if l.startswith("station 1 ")] == ["station 1 (+0.0 kHz): RDS PI 0x54A9 (WAAB)", 'station 1 (+0.0 kHz): RDS PS "WAAB 1  "'], lines
    assert not [l for l in lines if l.startswith("station 2 ")]
