"""GPU: the wideband receiver delivers every station's Station Information Guide and LOT files -- album art, station logos
(WidebandReceiver(data_services=True), nrsc5hip_aas_feed over all stations in one call per push, `python -m nrsc5_amd.wideband --dump-aas-files`).
Every station's events are compared with the SIG / LOT events the UNMODIFIED reference reports through its public API on the very bytes that
station's engine stream decoded (the channelizer's output, copied back)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import aas_args as aa, aas_model as am, psd_args as pa

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the generators carry 160 PSD bytes per frame: two tags and three times the SIG and the file are about 750 bytes, and a station's first frame may be lost
RATE, FMT, OFFS, LEVELS, N_FRAMES = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8], 5
KINDS = ("sig", "lot_header", "lot", "stream", "packet")
_cache = {}


def _sig(k):
    return aa.sig_service(10 + k) + aa.sig_name(b"ART%d" % k) + aa.sig_data(k, aa.LOT_PORT + k, 3, aa.MIME_ART)


def _file(k):
    return bytes((37 * k + 11 * j) & 0xff for j in range(100 + 9 * k)), b"cover%d.jpg" % k


def _psd_stream(k):
    """a different stream per station: two ID3 tags, each followed by the station's SIG and its file -- the header in its single fragment --, and both once
    more: a receiver that loses the first L1 frame (the reference does, at times) still meets a SIG in front of a whole file"""
    body, name = _file(k)
    lot = (aa.LOT_PORT + k, 7, aa.lot_packet(40 + k, 0, body, aa.lot_header(len(body), aa.MIME_ART, name)))
    sig = (aa.SIG_PORT, 1, _sig(k))
    tag = lambda j: (0x5100, 10 * k + j, pa.id3_tag("Station %d song %d" % (k, j), "Artist %d" % k))
    return b"".join(pa.hdlc(pa.aas_payload(*p)) for p in (tag(0), sig, lot, tag(1), sig, lot, sig, lot))


def _scene(hip_lib, reflib):
    """the 2.4 MS/s cu8 three-station scene of tests/test_gpu_wideband_metadata.py, every station with a SIG, tags and a file of its own, and the
    reference's public-API SIG / LOT events on every station's channelized stream"""
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
            R = am.RefAas(reflib)
            try:
                exp.append([e for e in R.run_iq(np.ascontiguousarray(y[s].reshape(-1))) if e[0] != "lot_fragment"])
            finally:
                R.close()
            kinds = [e[0] for e in exp[s]]
            assert kinds.count("sig") == 1 and kinds.count("lot") >= 1, (s, kinds)          # on the reference alone
            assert next(e for e in exp[s] if e[0] == "lot")[7] == _file(s)[0]
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
    """a reference event (aas_model.RefAas) as the fields the receiver logs"""
    if e[0] == "sig":
        out = []
        for kind, number, name, comps in e[1]:
            cs = []
            for ctype, cid, port, sdt, dtype, mime in comps:
                c = {"type": ctype, "id": cid, "port": port, "data_type": dtype, "mime": mime}
                if ctype == "data":
                    c["service_data_type"] = sdt
                cs.append(c)
            out.append({"type": kind, "number": number, "name": None if name is None else name.decode(), "components": cs})
        return "sig", out
    kind, port, lot, size, mime, name, expiry, data = e
    f = {"port": port, "lot": lot, "size": size, "mime": mime, "name": name.decode("latin-1"), "expiry": expiry}
    if kind == "lot":
        f["data"] = data
    return kind, f


def _same_logs(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb and va.keys() == vb.keys(), (ka, kb)
        for key in va:
            assert np.asarray(va[key]).tobytes() == np.asarray(vb[key]).tobytes(), (ka, key)


def test_gpu_every_station_delivers_the_reference_s_sig_and_files(hip_lib, reflib):
    cap, exp = _scene(hip_lib, reflib)
    seen, files = [], []
    rx, events = _receive(cap, hip_lib, data_services=True, on_aas=lambda *a: seen.append(a), on_file=lambda s, f: files.append((s, f["lot"])))
    meta, _ = _receive(cap, hip_lib, metadata=True)
    try:
        moved = 16 * rx.pushes
        for s in range(len(OFFS)):
            mine = [(k, v) for k, v in rx.logs[s] if k in KINDS]
            want = [_ref_fields(e) for e in exp[s]]
            assert mine == want, (s, [k for k, _ in mine], [k for k, _ in want])
            assert [(k, v) for t, k, v in events if t == s and k in KINDS] == mine
            lots = [v for k, v in want if k == "lot"]
            assert rx.files[s] == {(v["port"], v["lot"]): v for v in lots} and [f for f in files if f[0] == s] == [(s, v["lot"]) for v in lots]
            assert rx.services[s] == want[0][1] and rx.data.sig(s) == want[0][1] and rx.services[s][0]["name"] == "ART%d" % s
            # the ID3 path is the one of metadata=True
            id3 = [v for k, v in rx.logs[s] if k == "id3"]
            assert id3 == [v for k, v in meta.logs[s] if k == "id3"] and len(id3) >= 1 and rx.now_playing[s] == meta.now_playing[s]
            assert rx.aas[s] == [] and len(meta.aas[s]) >= 2 and all(a[2] == 0x5100 for a in seen if a[0] == s)
            # what crossed: 16 bytes per push, and per event 48 bytes and its data padded to 4 -- no fragment except inside its complete file
            pad = lambda n: 48 + (n + 3) // 4 * 4
            moved += sum(pad(len(a[4])) for a in seen if a[0] == s) + pad(len(am.run([(aa.SIG_PORT, 0, _sig(s))])[0][0][0][4]))
            moved += sum(pad(len(v["name"]) + (v["size"] if k == "lot" else 0)) for k, v in mine if k != "sig")
            st = rx.data.stats(s)
            assert st["lot_files"] == len(lots) and st["lot_fragments"] >= len(lots) and st["psd"] == sum(1 for a in seen if a[0] == s)
            assert {x: v for x, v in rx.psd.stats(s).items() if x != "d2h_bytes"} == {x: v for x, v in meta.psd.stats(s).items() if x != "d2h_bytes"}
        assert rx.data.stats(0)["d2h_bytes"] <= moved
        # data_services=True changes nothing else
        plain, _ = _receive(cap, hip_lib)
        assert plain.psd is None and plain.data is None and plain.files == [{} for _ in OFFS]
        for s in range(len(OFFS)):
            _same_logs(plain.logs[s], [e for e in rx.logs[s] if e[0] != "id3" and e[0] not in KINDS])
        plain.close()
    finally:
        rx.close()
        meta.close()


def test_gpu_cli_dump_aas_files(hip_lib, reflib, tmp_path):
    cap, exp = _scene(hip_lib, reflib)
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    out = tmp_path / "aas"
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE),
           "--offsets", ",".join(str(o) for o in OFFS), "--chunk", str(1 << 20), "--dump-aas-files", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    for s in range(len(OFFS)):
        lot = next(e for e in exp[s] if e[0] == "lot")
        path = out / ("station%d_%+d_%d_%s" % (s, int(round(OFFS[s])), lot[2], lot[5].decode()))
        assert path.read_bytes() == lot[7] == _file(s)[0]
        mine = [l.split(": ", 1)[1] for l in lines if l.startswith("station %d " % s)]
        assert "LOT file: port=%04X lot=%d name=%s size=%d mime=%08X expiry=2031-05-17T21:59:00Z" % (lot[1], lot[2], lot[5].decode(), lot[3], lot[4]) in mine
        assert "SIG Service: type=data number=%d name=ART%d" % (10 + s, s) in mine
        assert "  Data component: id=%d port=%04X service_data_type=260 type=3 mime=%08X" % (s, aa.LOT_PORT + s, aa.MIME_ART) in mine
    assert sorted(p.name for p in out.iterdir()) == sorted("station%d_%+d_%d_cover%d.jpg" % (s, int(round(OFFS[s])), 40 + s, s) for s in range(len(OFFS)))
