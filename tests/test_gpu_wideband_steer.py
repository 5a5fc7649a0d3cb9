"""GPU: the receiver steers every station's analog audio by its own reception (WidebandReceiver(steer=True); `python -m nrsc5_amd.wideband --steer
--dump-analog`).  The four-station 2.4 MS/s cu8 scene of tests/test_gpu_wideband_carrier.py, one L1 frame long, with both analog-only stations in
stereo: the one at 0 at about 40 dB in-filter CNR, the one at +400 kHz at about 12 dB.  The strong station's audio is that of a receiver without
steering, byte for byte, from audio block 18 on for as long as it transmits (the capture runs on for a few blocks behind the end of the
transmissions, where every carrier fades: the windowed CNR of the last block reads 20 dB); the weak one's is mono (L == R) where the unsteered
receiver plays the hiss of the difference channel; the snapshots are the factors nrsc5hip_stage_fm_steer gives for the same channelized streams."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import fm_model as fm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, CHUNK = 2400000, "cu8", 1 << 19
STEREO = dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2, 0.5)], preemph_us=75)
# offset, kind, host, cfo of the transmitter, level
SCENE = [(-600e3, "hd", STEREO, 400.0, 1.0), (0.0, "analog", STEREO, 1200.0, 1.0), (400e3, "analog", STEREO, -300.0, 0.039), (800e3, "hd", None, -700.0, 0.7)]
OFFSETS = [o for o, _, _, _, _ in SCENE]
STRONG, WEAK = 1, 2
S0 = fm.BLOCK_OUT * 18
_cache = {}


def _scene():
    if "cap" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=cfo, level=a, timing=977 * k, host=h, host_db=14.0, digital=kind == "hd")
              for k, (o, kind, h, cfo, a) in enumerate(SCENE)]
        _cache["cap"] = sw.capture(st, RATE, FMT, n_frames=1, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
    return _cache["cap"]


def _receive(hip_lib, **kw):
    from nrsc5_amd import wideband
    cap = _scene()
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFSETS, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, **kw)
    events, snaps, carriers = [], [], []
    for p in range(0, n, CHUNK):
        events += rx.push(cap.raw[2 * p:2 * min(n, p + CHUNK)])
        snaps.append(rx.steer)
        carriers.append(rx.carrier)
    return rx, events, (snaps, carriers)


def _stage_factors(hip_lib):
    """(q, b, h, g) of every audio block of the four channelized streams, through the stage hook"""
    cap = _scene()
    ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFSETS, lib_path=hip_lib)
    y = ch.process_tensor(cap.raw)
    D = eng.FmDemod(4, lib_path=hip_lib, steer=True)
    fac = D.stage_steer(y.data_ptr(), 2 * y.shape[1], y.shape[1])
    D.close(); ch.close()
    return fac


def _runs(hip_lib):
    from nrsc5_amd import wideband
    if "runs" not in _cache:
        rx, events, (snaps, carriers) = _receive(hip_lib, steer=True, carrier=True)
        plain, _, _ = _receive(hip_lib, analog=True)
        try:
            _cache["runs"] = dict(audio=[np.concatenate(a) for a in rx.audio], plain=[np.concatenate(a) for a in plain.audio], events=events, snaps=snaps,
                                  carrier=carriers, logs=(rx.logs, plain.logs), fac=_stage_factors(hip_lib),
                                  lines=[wideband.format_event(rx, s, k, v) for s, k, v in events if k == "steer"])
            assert plain.steer == [None] * 4 and rx.analog and rx.fm.steer_config is not None
        finally:
            plain.close()
            rx.close()
    return _cache["runs"]


def test_gpu_strong_station_is_untouched_and_weak_station_is_mono(hip_lib):
    r = _runs(hip_lib)
    cnr = [c["windowed"]["cnr_db"] for c in r["carrier"][2]]                                 # in the middle of the session
    print("windowed CNR of the four stations:", [round(c, 1) for c in cnr], "steer:", r["snaps"][2])
    assert cnr[STRONG] >= 35.0 and 9.0 <= cnr[WEAK] <= 15.0, cnr                            # the scene holds what it is named for
    a, p = r["audio"], r["plain"]
    assert all(x.shape == y.shape and x.shape[0] > 60000 for x, y in zip(a, p))
    full = np.all(r["fac"][STRONG][:, 1:] == 1.0, axis=1)                                    # blocks that end with every control at 1
    end = 18 + int(np.argmin(full[18:])) if not full[18:].all() else full.size               # the strong station: from block 18 to the end of its transmission
    print(f"the strong station holds every control at 1 from audio block 18 to {end} of {full.size}")
    assert full[17:end].all() and end >= full.size - 40
    assert a[STRONG][S0:fm.BLOCK_OUT * end].tobytes() == p[STRONG][S0:fm.BLOCK_OUT * end].tobytes() and np.abs(a[STRONG][S0:]).max() > 3000
    assert np.array_equal(a[WEAK][S0:, 0], a[WEAK][S0:, 1]) and not np.array_equal(p[WEAK][S0:, 0], p[WEAK][S0:, 1])
    assert np.abs(a[3]).max() < np.abs(p[3]).max()                                           # no host at all: muted
    for mine, theirs in zip(*r["logs"]):                                                     # the logs are those of a receiver without steering
        assert [k for k, _ in mine] == [k for k, _ in theirs]


def test_gpu_snapshots_are_the_stage_hooks_factors_and_events_are_rare(hip_lib):
    r = _runs(hip_lib)
    cap = _scene()
    fac = r["fac"]
    n, pos = cap.raw.numel() // 2, 0
    ch2 = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFSETS, lib_path=hip_lib)
    for i, p0 in enumerate(range(0, n, CHUNK)):
        pos += ch2.outputs_for(min(n, p0 + CHUNK) - p0)
        ch2.process_tensor(cap.raw[2 * p0:2 * min(n, p0 + CHUNK)])
        blocks = max(0, ((pos + 1) // 2) // fm.BLOCK - fm.W)
        for s in range(4):
            want = [float(v) for v in fac[s, blocks - 1]] if blocks else [0.0] * 4
            assert list(r["snaps"][i][s].values()) == want, (i, s, r["snaps"][i][s], want)
    ch2.close()
    mid, last = r["snaps"][2], r["snaps"][-1]
    assert mid[STRONG]["blend"] == 1.0 and mid[STRONG]["highcut"] == 1.0 and mid[STRONG]["mute"] == 1.0
    assert last[WEAK]["blend"] == 0.0 and 0.0 < last[WEAK]["highcut"] < 1.0 and last[WEAK]["mute"] == 1.0
    assert last[3]["blend"] == 0.0 and last[3]["highcut"] == 0.0 and last[3]["mute"] == np.float32(0.1)
    steer_events = [(s, v) for s, k, v in r["events"] if k == "steer"]
    assert {s for s, _ in steer_events} == {0, 1, 2, 3} and len(steer_events) <= 12, steer_events      # the first audio, then crossings only
    assert all(" reception blend " in l and " high-cut " in l and " mute " in l for l in r["lines"]), r["lines"]


def test_gpu_cli_steer_prints_reception_lines_and_writes_the_steered_audio(hip_lib, tmp_path):
    r = _runs(hip_lib)
    cap = _scene()
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    out = tmp_path / "wav"
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE), "--offsets", ",".join(str(o) for o in OFFSETS),
           "--chunk", str(CHUNK), "--dump-analog", str(out), "--blend-db", "18,30"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.decode().splitlines() if " reception " in l]
    assert lines == r["lines"], (lines, r["lines"])                           # --blend-db with the defaults implies --steer and changes nothing
    assert any(l.startswith("station 1 (+0.0 kHz): reception blend 1.00 high-cut 1.00 mute 1.00") for l in lines), lines
    assert any(l.startswith("station 2 (+400.0 kHz): reception blend 0.00 ") for l in lines), lines
    wavs = sorted(os.listdir(out))
    assert len(wavs) == 4 and all(w.endswith("_analog.wav") for w in wavs), wavs
    for s, w in enumerate(wavs):
        with wave.open(str(out / w), "rb") as h:
            assert (h.getnchannels(), h.getsampwidth(), h.getframerate()) == (2, 2, 44100)
            pcm = np.frombuffer(h.readframes(h.getnframes()), dtype=np.int16).reshape(-1, 2)
        assert pcm.tobytes() == r["audio"][s].tobytes(), w
