"""GPU: the wideband receiver plays every station's analog FM programme (WidebandReceiver(analog=True): nrsc5hip_chan_feed_fm, the demodulator
nrsc5hip_fm_* behind the channelizer's staged outputs; `python -m nrsc5_amd.wideband --dump-analog`).  The three-station 2.4 MS/s cu8 scene of
tests/test_gpu_wideband_metadata.py, one L1 frame long: the first station carries a stereo host, the second a mono host, the third none.  The
audio of the two hosted stations is compared with the float64 model (tests/fm_model.py) run on that station's channelized cs16
(Channelizer.process) by the rule of tests/fm_checks.py: no sample more than 1 LSB off, at most 1 % of the samples different, clip counts
equal.  The station without a host is not compared: its input is sidebands and noise, on which the discriminator is ill-conditioned."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import fm_args as fa, fm_model as fm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
HOSTS = [dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2, 0.5)], preemph_us=75),
         dict(left=[(2000.0, 0.3)], right=[(2000.0, 0.3)], pilot=None, preemph_us=75),
         None]
HOST_DB = 14.0
CHUNK = 1 << 20
_cache = {}


def _scene(hip_lib):
    """-> (capture, per hosted station: the model's (pcm, clips, info) on its channelized stream)"""
    if "scene" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)), host=h, host_db=HOST_DB)
              for k, (o, a, h) in enumerate(zip(OFFS, LEVELS, HOSTS))]
        cap = sw.capture(st, RATE, FMT, n_frames=1, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
        y = ch.process_tensor(cap.raw).cpu().numpy()
        ch.close()
        ha, tab = fa.tables(75.0)
        want = []
        for s in (0, 1):
            pcm, clips, info = fm.model(y[s], ha, tab)
            pcm32, _, _ = fm.model(y[s], ha, tab, dtype=np.float32)
            diff = np.abs(pcm.astype(np.int32) - pcm32.astype(np.int32))
            assert diff.max() <= 1 and np.mean(diff != 0) < fa.F32_SHARE_MAX, (s, diff.max(), np.mean(diff != 0))   # the reference's own estimate
            want.append((pcm, clips, info))
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


def _analog(hip_lib):
    if "rx" not in _cache:
        cap, _ = _scene(hip_lib)
        blocks = []
        rx, events = _receive(cap, hip_lib, analog=True, on_audio=lambda s, pcm: blocks.append((s, pcm)))
        audio = [np.concatenate(a) for a in rx.audio]
        _cache["rx"] = (audio, [list(l) for l in rx.logs], events, blocks, list(rx.stereo), list(rx.pilot), rx.fm.clip_counts(), rx.fm.latency_in)
        rx.close()
    return _cache["rx"]


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_hosted_stations_audio_equals_the_model(hip_lib):
    cap, want = _scene(hip_lib)
    audio, logs, events, blocks, stereo, pilot, clips, latency = _analog(hip_lib)
    for s in (0, 1):
        pcm, want_clips, info = want[s]
        assert audio[s].dtype == np.int16 and audio[s].shape == pcm.shape and pcm.shape[0] > 60000, (audio[s].shape, pcm.shape)
        diff = np.abs(audio[s].astype(np.int32) - pcm.astype(np.int32))
        print(f"station {s}: largest difference {diff.max()} LSB, {100 * np.mean(diff != 0):.4f} % of the samples differ, rms {np.sqrt(np.mean(pcm.astype(np.float64) ** 2)):.0f} LSB")
        assert diff.max() <= 1 and np.mean(diff != 0) <= 0.01, (s, diff.max(), np.mean(diff != 0))
        assert np.array_equal(clips[s], want_clips)
        assert stereo[s] == bool(info["stereo"][-1]) and abs(pilot[s] - info["level"][-1]) < 1e-5
    # every push's block went through on_audio, in order
    for s in range(len(OFFS)):
        assert np.array_equal(np.concatenate([b for t, b in blocks if t == s]), audio[s])
    # the count: what the definition gives for the station's stream
    assert audio[2].shape == audio[0].shape


def test_gpu_stereo_flag_and_tone_levels(hip_lib):
    _scene(hip_lib)
    audio, logs, events, blocks, stereo, pilot, clips, latency = _analog(hip_lib)
    lo, hi = fm.SETTLE, fm.SETTLE + 50000                       # inside the transmission: the capture ends with the carrier off
    # the flag at the end of the session belongs to the noise behind the transmission; the events say what it was while the station was on
    flags = [[v["stereo"] for k, v in logs[s] if k == "analog"] for s in range(len(OFFS))]
    assert flags[0][:1] == [True] and abs([v["pilot"] for k, v in logs[0] if k == "analog"][0] - 0.1) < 0.01
    for s in range(len(OFFS)):                                   # the events push() returned are the log's
        assert [v for t, k, v in events if t == s and k == "analog"] == [v for k, v in logs[s] if k == "analog"]
    assert True not in flags[1]                                 # the mono host never lights the flag
    a, b = audio[0][lo:hi], audio[1][lo:hi]
    for f, on, level in ((1000.0, 0, 0.3), (3000.0, 1, 0.2)):
        amp_db = 20 * np.log10(fm.tone(a[:, on], f, 0) / (0.9 * level * 32767))
        sep = 20 * np.log10(fm.tone(a[:, on], f, 0) / fm.tone(a[:, 1 - on], f, 0))
        print(f"stereo host: {f:.0f} Hz {amp_db:+.3f} dB, separation {sep:.1f} dB")
        assert abs(amp_db) <= 0.1 and sep >= 40.0, (f, amp_db, sep)
    assert np.array_equal(b[:, 0], b[:, 1])                     # mono host: L == R on every sample
    amp_db = 20 * np.log10(fm.tone(b[:, 0], 2000.0, 0) / (0.9 * 0.3 * 32767))
    print(f"mono host: 2000 Hz {amp_db:+.3f} dB")
    assert abs(amp_db) <= 0.1, amp_db


def test_gpu_digital_path_is_unaffected(hip_lib):
    cap, _ = _scene(hip_lib)
    audio, logs, events, blocks, stereo, pilot, clips, latency = _analog(hip_lib)
    plain, _ = _receive(cap, hip_lib)
    try:
        assert plain.fm is None and plain.audio == [[] for _ in OFFS]
        for s in range(len(OFFS)):
            assert len(plain.logs[s]) > 0
            _same_logs(plain.logs[s], [e for e in logs[s] if e[0] != "analog"])
        assert any(k == "sync" for k, v in plain.logs[2])
    finally:
        plain.close()


def test_gpu_cli_dump_analog(hip_lib, tmp_path):
    cap, _ = _scene(hip_lib)
    audio = _analog(hip_lib)[0]
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    out = tmp_path / "wav"
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(CHUNK), "--dump-analog", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    for s, o in enumerate(OFFS):
        path = out / f"station{s}_{int(round(o)):+d}_analog.wav"
        with wave.open(str(path), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, 44100)
            frames = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2)
        assert np.array_equal(frames, audio[s]), s
        assert any(l.startswith(f"station {s} ") and f"analog frames {len(frames)} " in l for l in lines), lines[-5:]
