"""GPU: the wideband receiver reports EAS alerts from every station's analog audio (WidebandReceiver(eas=True): FmDemod(same=True) behind the
channelizer's staged outputs; `python -m nrsc5_amd.wideband --eas`).  A three-station 2.4 MS/s cu8 scene, two L1 frames long (two header bursts
48 bits apart are 976 bits, 1.9 s): the first station carries a stereo host with the two bursts in its audio, the second a host with tones only,
the third no host.  Two equal bursts make a message: it must appear on the first station only, with the fields that were sent, and the receiver's
eas[s], the command line's line and the demodulator's snapshot must agree.  The record logs and the audio are those of a receiver without it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth_fm as sf

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
TEXT = "ZCZC-WXR-TOR-029095-029097+0030-1231405-KXYZ/FM -"
T_BIT = 1.0 / sf.SAME_BIT_HZ
BURST_BITS = 8 * (16 + len(TEXT))
STARTS = [0.05, 0.05 + (BURST_BITS + 48) * T_BIT]
HOSTS = [dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2, 0.5)], preemph_us=75, same=dict(bursts=[(t, TEXT) for t in STARTS], level=0.3)),
         dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2)], preemph_us=75),
         None]
HOST_DB = 14.0
CHUNK = 1 << 20
LINE = "station 0 (-800.0 kHz): EAS WXR TOR 029095,029097 +0030 day 123 14:05 KXYZ/FM"
_cache = {}


def _scene():
    if "scene" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)), host=h, host_db=HOST_DB)
              for k, (o, a, h) in enumerate(zip(OFFS, LEVELS, HOSTS))]
        _cache["scene"] = sw.capture(st, RATE, FMT, n_frames=2, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
    return _cache["scene"]


def _receive(cap, hip_lib, **kw):
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFS, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, **kw)
    events = []
    for p in range(0, n, CHUNK):
        events += rx.push(cap.raw[2 * p:2 * min(n, p + CHUNK)])
    return rx, events


def _eas(hip_lib):
    if "rx" not in _cache:
        rx, events = _receive(_scene(), hip_lib, analog=True, eas=True)
        _cache["rx"] = ([np.concatenate(a) for a in rx.audio], [list(l) for l in rx.logs], events, [list(e) for e in rx.eas],
                        [rx.fm.same_get(s) for s in range(len(OFFS))], [rx.fm.same_stats(s) for s in range(len(OFFS))])
        rx.close()
    return _cache["rx"]


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_message_on_the_station_that_sent_it(hip_lib):
    assert (STARTS[1] - STARTS[0]) / T_BIT - BURST_BITS == pytest.approx(48.0) and STARTS[1] + BURST_BITS * T_BIT < 2 * 1.486 - 0.2
    audio, logs, events, eas, snaps, stats = _eas(hip_lib)
    got = [(s, v) for s, k, v in events if k == "eas"]
    assert len(got) == 1 and got[0][0] == 0 and eas == [[got[0][1]], [], []]
    v = got[0][1]
    assert v["text"] == TEXT and v["kind"] == "header" and v["bursts"] == 2 and v["last"] - v["first"] == 8 * len(TEXT) - 1
    assert v["fields"] == eng.same_fields(TEXT) == {"originator": "WXR", "event": "TOR", "locations": ["029095", "029097"], "purge_minutes": 30, "day": 123,
                                                   "hour": 14, "minute": 5, "sender": "KXYZ/FM"}
    # the demodulator's snapshot is that message; the bursts were counted, and their events stayed on the device
    assert snaps[0]["text"] == TEXT.encode() and snaps[0]["kind"] == "header" and (snaps[0]["first"], snaps[0]["last"]) == (v["first"], v["last"])
    assert snaps[0]["group_bursts"] == 2 and stats[0]["bursts"] == 2 and stats[0]["messages"] == 1 and stats[0]["events"] == 1 and stats[0]["bursts_aborted"] == 0
    # tones only, and no host: bits, no burst, no message
    for s in (1, 2):
        assert snaps[s]["text"] is None and stats[s]["bursts"] == 0 and stats[s]["events"] == 0 and stats[s]["bits"] > 1000
    assert not any(k == "eas" for log in logs for k, _ in log)              # an event of the push, not of the record log


def test_gpu_eas_off_changes_nothing(hip_lib):
    cap = _scene()
    audio, logs, events, eas, snaps, stats = _eas(hip_lib)
    plain, plain_events = _receive(cap, hip_lib, analog=True)
    try:
        assert plain.eas == [[] for _ in OFFS] and not any(k == "eas" for _, k, _ in plain_events)
        for s in range(len(OFFS)):
            assert np.concatenate(plain.audio[s]).tobytes() == audio[s].tobytes(), s
            _same_logs(plain.logs[s], logs[s])
        with pytest.raises(eng.Nrsc5HipError):
            plain.fm.same_get(0)
    finally:
        plain.close()


def test_gpu_cli_eas_line(hip_lib, tmp_path):
    cap = _scene()
    audio, logs, events, eas, snaps, stats = _eas(hip_lib)
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(CHUNK), "--eas"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if " EAS " in l]
    assert lines == [LINE] == ["station 0 (-800.0 kHz): " + eng.same_line(eas[0][0]["text"])], lines
    assert eng.same_line(snaps[0]["text"]) in LINE
