"""GPU: the wideband receiver says what every station is playing (WidebandReceiver(metadata=True), nrsc5hip_psd_feed over all stations in one
call per push, `python -m nrsc5_amd.wideband --metadata`).  Every station's AAS packets are compared with the `l2aas` records of the UNMODIFIED
reference run on the very bytes that station's engine stream decoded (the channelizer's output, copied back)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from oracle import ref
from tests import psd_args as pa, psd_model as pm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS, N_FRAMES = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8], 3
_cache = {}


def _titles(k):
    return ["Station %d song %d ~}" % (k, j) for j in range(6)]


def _psd_stream(k):
    """a different stream per station: ID3 packets for program 0, a packet on another port behind the second one"""
    out = b""
    for j, title in enumerate(_titles(k)):
        out += pa.hdlc(pa.aas_payload(0x5100, 10 * k + j, pa.id3_tag(title, "Artist %d" % k, utf16=(j + k) % 3 == 2)), or_escape=j % 2 == 1)
        if j == 1:
            out += pa.hdlc(pa.aas_payload(0x0810 + k, 99, bytes(range(40 + k))))
    return out


def _sent_tags(k):
    """the tags the generator really transmits for station k: the packets complete within the 160 bytes per frame that N_FRAMES frames carry"""
    from nrsc5_amd import synth, wideband
    sent = _psd_stream(k)[:synth.PSD_PER_FRAME * N_FRAMES]
    return [wideband.parse_id3(data) for _, port, _, data in pm.PsdModel().push_bytes(0, sent) if port == 0x5100]


def _scene(hip_lib, reflib):
    """the 2.4 MS/s cu8 three-station scene of tests/test_gpu_wideband_programs.py, every station with a PSD stream of its own, and the reference's
    l2aas records of every station's channelized stream"""
    if "scene" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)), psd=_psd_stream(k))
              for k, (o, a) in enumerate(zip(OFFS, LEVELS))]
        cap = sw.capture(st, RATE, FMT, n_frames=N_FRAMES, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
        y = ch.process_tensor(cap.raw).cpu().numpy()
        ch.close()
        exp = []
        for s in range(len(OFFS)):
            log, _, _ = reflib.run(np.ascontiguousarray(y[s].reshape(-1)), taps=ref.TAP_L2)
            exp.append([v["data"] for k, v in log if k == "l2aas"])
            assert len(exp[s]) >= 3, (s, len(exp[s]))                 # on the reference alone
        assert len({tuple(e) for e in exp}) == len(OFFS)              # the stations carry different packets
        _cache["scene"] = (cap, exp)
    return _cache["scene"]


def _receive(cap, hip_lib, **kw):
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFS, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, **kw)
    events = []
    for p in range(0, n, 1 << 20):
        events += rx.push(cap.raw[2 * p:2 * min(n, p + (1 << 20))])
    return rx, events


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_every_station_delivers_the_reference_packets_and_its_titles(hip_lib, reflib):
    from nrsc5_amd import wideband
    cap, exp = _scene(hip_lib, reflib)
    seen = []
    rx, events = _receive(cap, hip_lib, metadata=True, on_aas=lambda *a: seen.append(a))
    try:
        for s in range(len(OFFS)):
            got = [a for a in seen if a[0] == s]
            assert [pm.packet_bytes(a) for a in got] == exp[s], (s, len(got), len(exp[s]))
            assert all(a[1] == 0 for a in got)
            # what the packets say: the tags in order as id3 events, the last one in now_playing, the other port raw
            tags = [wideband.parse_id3(d[4:]) for d in exp[s] if d[:2] == b"\x00\x51"]
            id3 = [v for k, v in rx.logs[s] if k == "id3"]
            assert id3 == [{"program": 0, **t} for t in tags] and len(tags) >= 2
            # the generator's titles, in its order (which frames a station decodes is the reference's word, not the generator's)
            where = [_titles(s).index(t["title"]) for t in tags]
            assert where == sorted(where) and all(t["artist"] == "Artist %d" % s for t in tags)
            assert rx.now_playing[s] == {0: tags[-1]}
            # ... and that is the generator's last title: the tags that arrived are the tail of what it transmitted (the stations' first L1 frame is
            # not always decoded, by the reference either), ending with the last tag complete in the transmitted bytes
            sent = _sent_tags(s)
            assert len(sent) >= 4 and tags == sent[-len(tags):] and rx.now_playing[s][0]["title"] == sent[-1]["title"] == _titles(s)[len(sent) - 1]
            assert rx.aas[s] == [(0, d[0] | d[1] << 8, d[2] | d[3] << 8, d[4:]) for d in exp[s] if d[:2] != b"\x00\x51"]
            assert rx.psd.stats(s)["delivered"] == len(exp[s])
        # the events push() returned: each station's id3 events are among them, in order
        for s in range(len(OFFS)):
            assert [v for t, k, v in events if t == s and k == "id3"] == [v for k, v in rx.logs[s] if k == "id3"]
        # the frames stayed on the device: what the feeds copied is the packets and a few words per call
        total = sum(len(d) for e in exp for d in e)
        assert rx.psd.stats(0)["d2h_bytes"] <= total + 16 * sum(len(e) for e in exp) + 256 * len(OFFS) * rx.pushes
        # metadata=True changes nothing else
        plain, _ = _receive(cap, hip_lib)
        assert plain.psd is None and plain.now_playing == [{} for _ in OFFS]
        for s in range(len(OFFS)):
            _same_logs(plain.logs[s], [e for e in rx.logs[s] if e[0] != "id3"])
        plain.close()
    finally:
        rx.close()


def test_gpu_cli_metadata(hip_lib, reflib, tmp_path):
    cap, exp = _scene(hip_lib, reflib)
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(1 << 20), "--metadata"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    for s in range(len(OFFS)):
        n = sum(1 for d in exp[s] if d[:2] == b"\x00\x51")
        mine = [l for l in lines if l.startswith("station %d " % s) and " ID3 program 0 " in l]
        assert len(mine) == n, (s, mine)
        from nrsc5_amd import wideband
        first = wideband.parse_id3(next(d for d in exp[s] if d[:2] == b"\x00\x51")[4:])
        assert "title=%r" % first["title"] in mine[0] and "artist='Artist %d'" % s in mine[0]
