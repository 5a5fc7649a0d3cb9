"""GPU: the scan finds analog-only stations and the receiver measures every station's carrier (wideband.scan(analog=True), confirm_analog,
WidebandReceiver(carrier=True); `python -m nrsc5_amd.wideband --scan-analog --dump-analog --carrier`).  One 2.4 MS/s cu8 scene, one L1 frame long:
a hybrid station with a stereo host at -600 kHz, an analog-only stereo station at 0 whose transmitter is 1.2 kHz off, an analog-only mono station
of about 15 dB in-filter CNR at +400 kHz and a hybrid station without a host at +800 kHz.  The figures are compared with the float64 model
(tests/carrier_model.py) run on the station's channelized cs16 (Channelizer.process), the receiver's snapshots bit for bit with the model's sums
of the device's own block triples of the same stream (nrsc5hip_stage_fm_carrier)."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import carrier_checks as cc, carrier_model as cm, fm_args as fa

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, CHUNK = 2400000, "cu8", 1 << 20
STEREO = dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2, 0.5)], preemph_us=75)
MONO = dict(left=[(2000.0, 0.3)], right=[(2000.0, 0.3)], pilot=None, preemph_us=75)
# offset, kind, host, cfo of the transmitter, level
SCENE = [(-600e3, "hd", STEREO, 400.0, 1.0), (0.0, "analog", STEREO, 1200.0, 0.8), (400e3, "analog", MONO, -300.0, 0.055), (800e3, "hd", None, -700.0, 0.7)]
HOST_DB = 14.0
_cache = {}


def stations():
    from nrsc5_amd import synth_wideband as sw
    return [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=cfo, level=a, timing=977 * k, host=h, host_db=HOST_DB, digital=kind == "hd")
            for k, (o, kind, h, cfo, a) in enumerate(SCENE)]


def carrier_hz(k: int) -> float:
    """where station k's analog carrier lies in the capture: the transmitter's offset moves it down (synth_wideband.capture)"""
    return SCENE[k][0] - SCENE[k][3]


def _scene():
    if "cap" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        cap = sw.capture(stations(), RATE, FMT, n_frames=1, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        assert [len(p) for p in cap.p1] == [1, 0, 0, 1] and [len(p) for p in cap.pids] == [16, 0, 0, 16]      # index-aligned, empty for the analog-only ones
        _cache["cap"] = cap
    return _cache["cap"]


def _found(hip_lib):
    if "found" not in _cache:
        from nrsc5_amd import wideband
        cap = _scene()
        _cache["found"] = wideband.scan(cap.raw, cap.rate, cap.fmt, analog=True, lib_path=hip_lib)
        for s in _cache["found"]:
            print(wideband.format_found(s))
    return _cache["found"]


def _channelized(hip_lib, centres, n=None):
    cap = _scene()
    ch = eng.Channelizer(cap.rate, eng.IQ_CU8, centres, lib_path=hip_lib)
    x = cap.raw if n is None else cap.raw[:2 * n]
    y = ch.process_tensor(x)
    ch.close()
    return y


def test_gpu_scan_finds_both_kinds_and_nothing_else(hip_lib):
    found = _found(hip_lib)
    assert [s.kind for s in found] == [k for _, k, _, _, _ in SCENE], [(s.offset_hz, s.kind) for s in found]
    for k, s in enumerate(found):
        o = SCENE[k][0]
        assert abs(s.offset_hz - o) < 2500.0, (k, s.offset_hz)                       # nothing at a hybrid's sidebands: exactly the four
        assert s.cnr_db is not None and s.level_db is not None and np.isfinite(s.cnr_db)
        if SCENE[k][2] is not None:
            assert abs(s.offset_hz + s.carrier_offset_hz - carrier_hz(k)) <= 200.0, (k, s.offset_hz, s.carrier_offset_hz, carrier_hz(k))
            assert s.cnr_db >= 10.0
    assert found[0].psmi is not None and found[3].psmi is not None and found[1].psmi is None
    assert found[3].cnr_db == cm.DB_MIN or found[3].cnr_db < 0.0                         # a hybrid without a host: no carrier
    assert found[0].stereo and found[1].stereo and not found[2].stereo
    assert abs(found[1].offset_hz - carrier_hz(1)) < 300.0                               # the analog-only centre was corrected onto the carrier


def test_gpu_mono_station_cnr_equals_the_model(hip_lib):
    found = _found(hip_lib)
    cap = _scene()
    n = int(1.0 * RATE)                                                                   # the confirmation window
    y = _channelized(hip_lib, [found[2].offset_hz], n).cpu().numpy()[0]
    _, _, t = cm.front(y, fa.tables()[0])
    want = cm.reports(t)["running"]
    print(f"mono station: scan cnr {found[2].cnr_db:.2f} dB level {found[2].level_db:.2f} dBFS, model {want['cnr_db']:.2f} dB {want['level_db']:.2f} dBFS")
    assert 12.0 <= want["cnr_db"] <= 18.0                                                 # the scene holds what it is named for
    assert abs(found[2].cnr_db - want["cnr_db"]) <= 1.5


def _receive(hip_lib, offsets, **kw):
    from nrsc5_amd import wideband
    cap = _scene()
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offsets, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, **kw)
    events, snaps = [], []
    for p in range(0, n, CHUNK):
        events += rx.push(cap.raw[2 * p:2 * min(n, p + CHUNK)])
        snaps.append(rx.carrier)
    return rx, events, snaps


def test_gpu_receiver_snapshots_and_untouched_logs(hip_lib):
    from nrsc5_amd import wideband
    offsets = [s.offset_hz for s in _found(hip_lib)]
    rx, events, snaps = _receive(hip_lib, offsets, carrier=True)
    plain, _, _ = _receive(hip_lib, offsets)
    try:
        assert plain.fm is None and plain.carrier == [None] * 4 and rx.fm is not None and rx.audio == [[] for _ in offsets]
        for s in range(4):
            assert len(plain.logs[s]) == len(rx.logs[s])
            for (ka, va), (kb, vb) in zip(plain.logs[s], rx.logs[s]):
                assert ka == kb and va.keys() == vb.keys()
                for key in va:
                    assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (s, ka, key)
        assert any(k == "sync" for k, v in rx.logs[0]) and any(k == "sync" for k, v in rx.logs[3]) and not any(k == "sync" for k, v in rx.logs[1])
        # the snapshots: the stated sums of the device's block triples of the same streams, after every push
        y = _channelized(hip_lib, offsets)
        D = eng.FmDemod(4, lib_path=hip_lib)
        _, t = D.stage_carrier(y.data_ptr(), 2 * y.shape[1], y.shape[1])
        D.close()
        n = _scene().raw.numel() // 2
        ch = eng.Channelizer(_scene().rate, eng.IQ_CU8, offsets, lib_path=hip_lib)
        pos = 0
        for i, p in enumerate(range(0, n, CHUNK)):
            pos += ch.outputs_for(min(n, p + CHUNK) - p)
            ch.process_tensor(_scene().raw[2 * p:2 * min(n, p + CHUNK)])
            for s in range(4):
                cc.assert_report(snaps[i][s], t[s], ((pos + 1) // 2) // cm.BLOCK, (i, s))
        ch.close()
        # ... and the float64 model's figures on those streams
        yh = y.cpu().numpy()
        for s in (0, 1, 2):
            want = cm.reports(cm.front(yh[s], fa.tables()[0])[2])
            for kind in ("windowed", "running"):
                assert abs(snaps[-1][s][kind]["cnr_db"] - want[kind]["cnr_db"]) <= 0.05 and abs(snaps[-1][s][kind]["offset_hz"] - want[kind]["offset_hz"]) <= 1.0
        lines = [wideband.format_event(rx, s, k, v) for s, k, v in events if k == "carrier"]
        assert lines and all(" carrier " in l and " CNR " in l and " offset " in l for l in lines), lines[:3]
        assert {s for s, k, v in events if k == "carrier"} == {0, 1, 2, 3}
    finally:
        plain.close()
        rx.close()


def test_gpu_cli_scan_analog_dumps_four_stations(hip_lib, tmp_path):
    cap = _scene()
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    out = tmp_path / "wav"
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE), "--scan-analog", "--chunk", str(CHUNK),
           "--dump-analog", str(out), "--carrier"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    found = [l for l in lines if l.startswith("found ")]
    assert len(found) == 4 and sum(" analog " in l for l in found) == 2, found
    wavs = sorted(os.listdir(out))
    assert len(wavs) == 4 and all(w.endswith("_analog.wav") for w in wavs), wavs
    for w in wavs:
        with wave.open(str(out / w), "rb") as h:
            assert (h.getnchannels(), h.getsampwidth(), h.getframerate()) == (2, 2, 44100) and h.getnframes() > 60000
    assert any(" carrier " in l and " CNR " in l for l in lines if l.startswith("station 1 "))
