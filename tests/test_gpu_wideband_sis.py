"""GPU: the wideband receiver says who every station is (WidebandReceiver(sis=True), nrsc5hip_sis_feed over all stations in one call per push,
`python -m nrsc5_amd.wideband --sis`, scan(names=True)).  Every station's events are compared with the SIS events the UNMODIFIED reference
reports through its public API on the very bytes that station's engine stream decoded (the channelizer's output, copied back)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import sis_args as sa, sis_model as sm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, OFFS, LEVELS, N_FRAMES = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8], 3
_cache = {}


def _scene(hip_lib, reflib):
    """the 2.4 MS/s cu8 three-station scene of tests/test_gpu_wideband_metadata.py, every station with a SIS schedule and a name of its own, and
    the reference's public-API SIS events on every station's channelized stream"""
    if "scene" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        rng = np.random.default_rng(RATE)
        st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)),
                         pids=sa.schedule(k, never_complete=False)) for k, (o, a) in enumerate(zip(OFFS, LEVELS))]
        cap = sw.capture(st, RATE, FMT, n_frames=N_FRAMES, noise_rms=0.02, seed=3, device=torch.device("cuda", 0))
        ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFS, lib_path=hip_lib)
        y = ch.process_tensor(cap.raw).cpu().numpy()
        ch.close()
        exp = []
        for s in range(len(OFFS)):
            R = sm.RefSis(reflib)
            try:
                exp.append(list(R.run_iq(np.ascontiguousarray(y[s].reshape(-1)))))
            finally:
                R.close()
            # on the reference alone: a name, and enough events
            assert sum(1 for e in exp[s] if e[0] == "station_name") >= 1 and len(exp[s]) >= 5, (s, exp[s])
        assert len({tuple(e) for e in exp}) == len(OFFS)                # the stations differ
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


def _ref_fields(e):
    """a reference event (sis_model.RefSis) as the fields the receiver logs"""
    text = lambda b: None if b is None else b.decode("utf-8", errors="replace")
    kind = e[0]
    if kind == "station_id":
        return kind, {"country": e[1].decode(), "fcc": e[2]}
    if kind in ("station_name", "station_slogan", "station_message"):
        return kind, {kind[8:]: text(e[1])}
    if kind == "station_location":
        return kind, {"latitude": e[1], "longitude": e[2], "altitude": e[3]}
    if kind == "audio_service":
        return kind, dict(zip(("program", "access", "type", "sound_exp"), e[1:]))
    if kind == "data_service":
        return kind, dict(zip(("access", "type", "mime_type"), e[1:]))
    if kind == "alert":
        return kind, {"message": text(e[1]), "control_data": e[2]}
    if kind == "leap_second":
        return kind, dict(zip(("pending_offset", "current_offset", "pending_alfn"), e[1:]))
    if kind == "local_time":
        return kind, dict(zip(("utc_offset", "dst_regional", "dst_local", "dst_schedule"), e[1:]))
    d = {"manufacturer_id": e[1].decode("latin-1"), "core_version": list(e[2]), "manufacturer_version": list(e[4]), "core_status": e[3], "manufacturer_status": e[5]}
    if kind == "exciter":
        d["importer_connected"] = e[6]
    return kind, d


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_every_station_reports_the_reference_s_sis_events(hip_lib, reflib):
    cap, exp = _scene(hip_lib, reflib)
    rx, events = _receive(cap, hip_lib, sis=True)
    try:
        kinds = set(eng.SIS_KINDS[1:])
        info = rx.station_info
        for s in range(len(OFFS)):
            mine = [(k, v) for k, v in rx.logs[s] if k in kinds]
            want = [_ref_fields(e) for e in exp[s]]
            got = [(k, {"message": v["message"]}) if k == "station_message" else (k, v) for k, v in mine]      # (the priority is not in the reference's event)
            assert got == want, (s, len(got), len(want))
            # the events push() returned: the station's SIS events are among them, in order, behind the record events of their push
            assert [(k, v) for t, k, v in events if t == s and k in kinds] == mine
            # the snapshot: the model over the frames this station's records hold (one sync, no reset behind it), and what the last events said
            frames = [v["bits"] for k, v in rx.logs[s] if k == "pids"]
            assert sum(1 for k, v in rx.logs[s] if k == "sync") == 1
            m = sm.run(frames)[1]
            assert info[s] == m.info()
            assert info[s]["name"] == [v["name"] for k, v in mine if k == "station_name"][-1] is not None
            assert (info[s]["country"], info[s]["fcc"]) == (sa.STATIONS[s][1], sa.STATIONS[s][2])
            st = rx.sis.stats(s)
            assert st["events"] == len(mine) and st["frames"] == len(frames)
        assert len({i["name"] for i in info}) == len(OFFS)
        # only events crossed: 16 bytes of arena header per push and 48 bytes + the text per event
        total = sum(len(e) for e in exp)
        assert rx.sis.stats(0)["d2h_bytes"] <= 16 * rx.pushes + total * (eng.SIS_EVENT_HEADER + 384)
        # sis=True changes nothing else
        plain, _ = _receive(cap, hip_lib)
        assert plain.sis is None and plain.station_info == [None] * len(OFFS)
        for s in range(len(OFFS)):
            _same_logs(plain.logs[s], [e for e in rx.logs[s] if e[0] not in kinds])
        plain.close()
    finally:
        rx.close()


def test_gpu_cli_sis(hip_lib, reflib, tmp_path):
    cap, exp = _scene(hip_lib, reflib)
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(1 << 20), "--sis"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    words = {"station_id": "STATION_ID", "station_name": "STATION_NAME", "station_slogan": "STATION_SLOGAN", "station_message": "STATION_MESSAGE",
             "station_location": "STATION_LOCATION", "audio_service": "AUDIO_SERVICE", "data_service": "DATA_SERVICE", "alert": "ALERT",
             "leap_second": "LEAP_SECOND", "local_time": "LOCAL_TIME", "exciter": "EXCITER", "importer": "IMPORTER"}
    for s in range(len(OFFS)):
        mine = [l.split(": ", 1)[1] for l in lines if l.startswith("station %d " % s) and l.split(": ", 1)[1].split(" ")[0] in words.values()]
        assert [l.split(" ")[0] for l in mine] == [words[e[0]] for e in exp[s]], s
        name = next(e[1] for e in exp[s] if e[0] == "station_name").decode()
        assert "STATION_NAME %r" % name in mine and "STATION_ID country=%s facility_id=%d" % (sa.STATIONS[s][1], sa.STATIONS[s][2]) in mine


def test_gpu_scan_names_the_stations(hip_lib, reflib):
    from nrsc5_amd import wideband
    cap, exp = _scene(hip_lib, reflib)
    plain = wideband.scan(cap.raw, cap.rate, cap.fmt, lib_path=hip_lib)
    named = wideband.scan(cap.raw, cap.rate, cap.fmt, lib_path=hip_lib, names=True)
    assert len(plain) == len(named) == len(OFFS)
    for s, (a, b) in enumerate(zip(plain, named)):
        # without names: what the scan returned before there were names
        assert (a.name, a.country, a.facility_id, a.first_name_s) == (None, None, None, None)
        assert (a.offset_hz, a.score_db, a.lower_db, a.upper_db, a.floor_db, a.freq_offset_hz, a.psmi, a.pids_ok, a.first_pids_s) == \
               (b.offset_hz, b.score_db, b.lower_db, b.upper_db, b.floor_db, b.freq_offset_hz, b.psmi, b.pids_ok, b.first_pids_s)
        assert wideband.format_found(a) == wideband.format_found(b).rsplit(" name ", 1)[0] and " name " not in wideband.format_found(a)
        # with names: a name the reference reported for that station, its country and facility id
        assert b.name in [e[1].decode() for e in exp[s] if e[0] == "station_name"] and b.name.startswith(sa.STATIONS[s][0])
        assert (b.country, b.facility_id) == (sa.STATIONS[s][1], sa.STATIONS[s][2]) and 0 < b.first_name_s <= wideband.NAME_SECONDS
        assert wideband.format_found(b).endswith(" name " + b.name)
