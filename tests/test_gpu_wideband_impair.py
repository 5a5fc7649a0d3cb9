"""GPU: the receiver and the scan tell multipath and a neighbour on one side apart (WidebandReceiver(impair=True), wideband.scan(analog=True);
`python -m nrsc5_amd.wideband --impair`).  One 2.4 MS/s cu8 scene, one L1 frame (1.49 s) long, four analog-only stations: a clean one at -800 kHz,
one with a second ray (0.3, 5 us, 2.0) at -300 kHz, a weak and quietly modulated one at +400 kHz, and at +600 kHz its neighbour, 10 dB stronger and
modulated like an ordinary station.  The receiver's snapshots are compared bit for bit with the model's sums (tests/impair_model.py) of the device's
own block records of the same channelized stream (nrsc5hip_stage_fm_impair)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import impair_args as ia, impair_checks as ic, impair_model as im

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, FMT, CHUNK = 2400000, "cu8", 1 << 20
QUIET = dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2)], pilot=0.1, pilot_phase=0.7)
# offset, host, level, the verdict it is there for: (multipath, adjacent, side)
SCENE = [(-800e3, dict(ia.PROG), 1.0, (False, False, 0)), (-300e3, dict(ia.PROG, rays=[ia.RAY5]), 1.0, (True, False, 0)),
         (400e3, QUIET, 10 ** -0.5, (False, True, 1)), (600e3, dict(ia.NEIGHBOUR), 1.0, (False, False, 0))]
OFFSETS = [s[0] for s in SCENE]
_cache = {}


def _scene():
    if "cap" not in _cache:
        import torch
        from nrsc5_amd import synth_wideband as sw
        st = [sw.Station(offset_hz=o, seed=0, level=a, host=h, digital=False) for o, h, a, _ in SCENE]
        _cache["cap"] = sw.capture(st, RATE, FMT, n_frames=1, noise_rms=0.005, seed=5, device=torch.device("cuda", 0))
        raw = _cache["cap"].raw
        assert int(raw.min()) > 0 and int(raw.max()) < 255                   # nothing clips: clipping is an impairment of its own
    return _cache["cap"]


def _received(hip_lib):
    if "rx" not in _cache:
        from nrsc5_amd import wideband
        cap = _scene()
        n = cap.raw.numel() // 2
        rx = wideband.WidebandReceiver(cap.rate, cap.fmt, OFFSETS, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, lib_path=hip_lib, impair=True)
        events, snaps = [], []
        try:
            assert rx.analog and rx.fm is not None and rx.fm.carrier_enabled
            for p in range(0, n, CHUNK):
                events += rx.push(cap.raw[2 * p:2 * min(n, p + CHUNK)])
                snaps.append(rx.impair)
            lines = [wideband.format_event(rx, s, k, v) for s, k, v in events if k == "impair"]
        finally:
            rx.close()
        _cache["rx"] = (events, snaps, lines)
    return _cache["rx"]


def test_gpu_verdicts_are_clear_multipath_adjacent_upper_clear(hip_lib):
    events, snaps, lines = _received(hip_lib)
    for s, (_, _, _, want) in enumerate(SCENE):
        w = snaps[-1][s]["windowed"]
        print(f"station {s}: explained {w['explained']:.3f} depth {w['depth']:.3f} rho {w['rho']:+.3f} usn {w['usn_db']:.1f} dB ripple {w['ripple_db']:.1f} dB")
        assert (w["multipath"], w["adjacent"], w["side"]) == want, (s, w)
    assert snaps[-1][1]["windowed"]["explained"] >= 0.7 and snaps[-1][2]["windowed"]["rho"] >= 0.55 and abs(snaps[-1][3]["windowed"]["rho"]) <= 0.1


def test_gpu_snapshots_equal_the_stage_hook_after_every_push(hip_lib):
    _, snaps, _ = _received(hip_lib)
    cap = _scene()
    n = cap.raw.numel() // 2
    ch = eng.Channelizer(cap.rate, eng.IQ_CU8, OFFSETS, lib_path=hip_lib)
    y = ch.process_tensor(cap.raw)
    ch.reset()
    D = eng.FmDemod(4, lib_path=hip_lib)
    t = D.stage_impair(y.data_ptr(), 2 * y.shape[1], y.shape[1])["sums"]
    D.close()
    pos = 0
    for i, p in enumerate(range(0, n, CHUNK)):
        pos += ch.outputs_for(min(n, p + CHUNK) - p)
        ch.process_tensor(cap.raw[2 * p:2 * min(n, p + CHUNK)])
        for s in range(4):
            ic.assert_report(snaps[i][s], t[s], ((pos + 1) // 2) // im.BLOCK, (i, s))
    ch.close()
    assert pos == y.shape[1] and t.shape[1] > 900


def test_gpu_events_and_lines(hip_lib):
    events, snaps, lines = _received(hip_lib)
    mine = [(s, v) for s, k, v in events if k == "impair"]
    assert {s for s, _ in mine} == {0, 1, 2, 3}
    for s, (_, _, _, want) in enumerate(SCENE):
        vs = [v for st, v in mine if st == s]
        assert (vs[-1]["multipath"], vs[-1]["adjacent"], vs[-1]["side"]) == want, (s, vs)
        said = [(v["multipath"], v["adjacent"], v["side"]) for v in vs]
        assert all(a != b for a, b in zip(said, said[1:])), (s, said)          # only when a verdict bit changed
    print("\n".join(lines))
    last = {s: [l for l in lines if l.startswith(f"station {s} ")][-1] for s in range(4)}
    assert last[0] == "station 0 (-800.0 kHz): reception clear" and last[3] == "station 3 (+600.0 kHz): reception clear"
    assert last[1].startswith("station 1 (-300.0 kHz): reception multipath depth 0.") and "(explained 0." in last[1] and "adjacent" not in last[1]
    assert last[2].startswith("station 2 (+400.0 kHz): reception adjacent upper rho +0.") and last[2].endswith(" dB") and " usn -" in last[2]


def test_gpu_scan_carries_the_verdicts(hip_lib):
    from nrsc5_amd import wideband
    cap = _scene()
    found = wideband.scan(cap.raw, cap.rate, cap.fmt, analog=True, lib_path=hip_lib)
    for s in found:
        print(wideband.format_found(s))
    # every entry is one of the four stations, and every station is there (the spectrum detector may nominate a fully modulated station twice, and
    # both nominations are then corrected onto the same carrier: the detector is not this test's subject)
    at = [int(np.argmin([abs(s.offset_hz - o) for o in OFFSETS])) for s in found]
    assert all(s.kind == "analog" and abs(s.offset_hz - OFFSETS[k]) < 2500.0 for s, k in zip(found, at)) and set(at) == {0, 1, 2, 3}, [(s.offset_hz, s.kind) for s in found]
    for s, k in zip(found, at):
        assert (s.multipath, s.adjacent, s.adjacent_side) == SCENE[k][3], s
        assert all(np.isfinite(v) for v in (s.explained, s.depth, s.rho, s.usn_db))
        line = wideband.format_found(s)
        assert ("reception multipath" in line) == (k == 1) and ("reception adjacent upper" in line) == (k == 2) and ("reception" in line) == (k in (1, 2)), line


def test_gpu_cli_prints_the_reception_lines(hip_lib, tmp_path):
    cap = _scene()
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    cmd = [sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", FMT, "--rate", str(RATE), "--offsets=" + ",".join(str(o) for o in OFFSETS),
           "--chunk", str(CHUNK), "--impair"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if " reception " in l]
    assert lines == _received(hip_lib)[2], lines


def test_gpu_report_what_a_hybrid_stations_host_reads(hip_lib):
    """no gate but finite figures: a hybrid station's own digital sidebands lie on both sides, 129 .. 198 kHz from the carrier -- what they do to
    rho and usn_db is printed (DESIGN.md (t) keeps the figures)"""
    import torch
    from nrsc5_amd import synth_wideband as sw, wideband
    st = [sw.Station(offset_hz=0.0, seed=77, level=1.0, host=dict(ia.PROG), host_db=14.0), sw.Station(offset_hz=600e3, seed=0, level=1.0, host=dict(ia.PROG), digital=False)]
    cap = sw.capture(st, RATE, FMT, n_frames=1, noise_rms=0.005, seed=6, device=torch.device("cuda", 0))
    snaps, _, _, _ = wideband.measure_carriers(cap.raw, int(0.5 * RATE), cap.rate, eng.IQ_CU8, [0.0, 600e3], lib_path=hip_lib, impair=True)
    for name, snap in zip(("hybrid host", "analog-only"), snaps):
        w, c = snap["impair"]["windowed"], snap["windowed"]
        print(f"{name}: cnr {c['cnr_db']:.1f} dB explained {w['explained']:.3f} depth {w['depth']:.3f} rho {w['rho']:+.3f} usn {w['usn_db']:.1f} dB ripple {w['ripple_db']:.1f} dB "
              f"multipath {w['multipath']} adjacent {w['adjacent']}")
        assert all(np.isfinite(w[k]) for k in im.FIGURES)
