"""GPU: the band scan (nrsc5hip_scan_*) on the MI355X -- its spectrum against the float64 restatement (tests/scan_model.py), its
nominations on the synthetic scenes against the model's on the same bytes, the confirmation by decode (nrsc5_amd/wideband.py: scan),
and the CLI without --offsets against the CLI with them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import scan_model as sm
from tests.test_scan_cpu import REL_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    import torch
    return torch.device("cuda", 0)


def _push(sc, x, chunks):
    n, pos = x.numel() // 2, 0
    for c in chunks:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        sc.push_tensor(x[2 * pos:2 * (pos + c)])
        pos += c
    assert pos == n
    return sc.spectrum()[1]


@pytest.mark.parametrize("rate,fmt", [(2400000, eng.IQ_CU8), (10000000, eng.IQ_CS16), (10000000, eng.IQ_CF32), (20000000, eng.IQ_CS16),
                                      (20000000, eng.IQ_CF32)], ids=["2.4M-cu8", "10M-cs16", "10M-cf32", "20M-cs16", "20M-cf32"])
def test_gpu_device_equals_float64_model(hip_lib, rate, fmt):
    import torch
    n = 200000 + 4321
    raw = sm.noise_plus_tone(fmt, n, seed=rate // 1000 + fmt)
    sc = eng.Scanner(rate, fmt, lib_path=hip_lib)
    assert sc.nfft == sm.default_nfft(rate)
    got = _push(sc, torch.from_numpy(raw).to(_dev()), [n // 3, n - n // 3])
    assert sc.segments == sm.segments(n, sc.nfft)
    want = sm.psd(sm.scaled(raw, fmt), sc.nfft)
    sc.close()
    err = sm.rel_error(got, want)
    print(f"rate {rate} fmt {fmt} nfft {want.size}: largest relative error {err:.3e}")
    assert err <= REL_BOUND, err


@pytest.mark.parametrize("fmt", [eng.IQ_CU8, eng.IQ_CS16, eng.IQ_CF32], ids=["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("explicit", [True, False], ids=["explicit", "default"])
@pytest.mark.parametrize("rate,nfft", sm.EVEN_NFFT_CASES, ids=[str(c[1]) for c in sm.EVEN_NFFT_CASES])
def test_gpu_even_transform_sizes_equal_float64_model(hip_lib, rate, nfft, explicit, fmt):
    """nfft 1024 and 4096: radix-4 passes alone, and at 4096 more than 64 KiB of dynamic LDS; asked for by size and reached through the
    rate's default.  Measured on the twin and on the device alike: 1.1e-13 .. 4.7e-13."""
    import torch
    n = nfft // 2 * 15 + 37
    raw = sm.noise_plus_tone(fmt, n, seed=nfft + fmt)
    sc = eng.Scanner(rate, fmt, nfft=nfft if explicit else 0, lib_path=hip_lib)
    assert sc.nfft == nfft == sm.default_nfft(rate)
    got = _push(sc, torch.from_numpy(raw).to(_dev()), [n // 3, n - n // 3])
    assert sc.segments == sm.segments(n, nfft)
    sc.close()
    err = sm.rel_error(got, sm.psd(sm.scaled(raw, fmt), nfft))
    print(f"scan nfft {nfft} {'explicit' if explicit else 'default'} fmt {fmt}: largest relative error {err:.3e}")
    assert err <= REL_BOUND, err


@pytest.mark.parametrize("name", list(sm.MANY_SEGMENT_CASES))
def test_gpu_many_segments_per_push(hip_lib, name):
    """More than ROWS_TARGET segments in one push: every workgroup carries its sums across a run of segments (the last run is short),
    and "rows-over-target" clamps the run to RUN_MAX with more rows than ROWS_TARGET.  Measured on the device: 4.5e-14 .. 7.3e-14."""
    import torch
    nfft, n, fmt, chunks = sm.many_segment_pushes(name)
    raw = sm.noise_plus_tone(fmt, n, seed=nfft + len(name))
    x = torch.from_numpy(raw).to(_dev())
    sc = eng.Scanner(2400000, fmt, nfft=nfft, lib_path=hip_lib)
    got = _push(sc, x, chunks)
    assert sc.segments == sm.segments(n, nfft)
    err = sm.rel_error(got, sm.psd(sm.scaled(raw, fmt), nfft))
    print(f"scan {name}: largest relative error {err:.3e}")
    assert err <= REL_BOUND, err
    if name == "rows-over-target":                                    # the same pushes give the same bytes: the reduce adds 1094 rows in row order
        sc.reset()
        assert _push(sc, x, chunks).tobytes() == got.tobytes()
    sc.close()


def test_gpu_chunking_reset_and_repeatability(hip_lib):
    import torch
    rate, fmt, n = 10000000, eng.IQ_CS16, 150000
    raw = sm.noise_plus_tone(fmt, n, seed=9)
    x = torch.from_numpy(raw).to(_dev())
    rng = np.random.default_rng(7)
    ref = None
    for nfft in (0, 512):
        for chunks in ([n], [7] * 300 + [n], [nfft - 1 if nfft else 8191] * (n // 500 + 1), list(rng.integers(1, 20000, 200))):
            sc = eng.Scanner(rate, fmt, nfft=nfft, lib_path=hip_lib)
            a = _push(sc, x, chunks)
            assert sc.segments == sm.segments(n, sc.nfft)
            sc.reset()
            b = _push(sc, x, chunks)
            sc.close()
            assert a.tobytes() == b.tobytes()
            if ref is None or ref.size != a.size:
                ref = a
            else:
                assert sm.rel_error(a, ref) <= 1e-5


def _scene(name):
    raw, rate, fmt, true, cap = sm.scene(name, device=_dev())
    return raw, rate, fmt, true, cap


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_gpu_nominations_equal_the_models(hip_lib, name):
    raw, rate, fmt, true, _ = _scene(name)
    sc = eng.Scanner(rate, eng.IQ_FORMATS[fmt], lib_path=hip_lib)
    sc.push_tensor(raw)
    got = sc.detect()
    psd = sc.spectrum()[1]
    sc.close()
    model_psd = sm.psd(sm.scaled(raw.cpu().numpy(), eng.IQ_FORMATS[fmt]), psd.size)
    assert sm.rel_error(psd, model_psd) <= REL_BOUND
    want = sm.detect(model_psd, rate)
    bw = rate / psd.size
    print(name, [(round(g["offset_hz"] / 1e3, 1), round(g["score_db"], 1)) for g in got])
    assert sorted(round(g["offset_hz"] / bw) + psd.size // 2 for g in got) == sorted(w["bin"] for w in want)
    assert len(got) == len(true)
    for f in true:
        assert min(abs(g["offset_hz"] - f) for g in got) <= 1.5 * bw, (f, got)


def test_gpu_scan_confirms_the_eight_stations(hip_lib):
    from nrsc5_amd import wideband
    raw, rate, fmt, true, _ = _scene("B")
    found = wideband.scan(raw, rate, fmt, lib_path=hip_lib)
    print([(round(s.offset_hz / 1e3, 1), round(s.score_db, 1), s.psmi, s.pids_ok, s.first_pids_s) for s in found])
    bw = rate / sm.default_nfft(rate)
    assert len(found) == len(true) == 8
    for f, s in zip(sorted(true), found):
        assert abs(s.offset_hz - f) <= 1.5 * bw
        assert s.pids_ok >= 1 and s.psmi == 1 and abs(s.freq_offset_hz) < 13.8e3
    assert [s.offset_hz for s in wideband.scan(raw, rate, fmt, confirm=False, lib_path=hip_lib)] == [s.offset_hz for s in found]


def test_gpu_scan_rejects_the_phantom_between_analog_carriers(hip_lib):
    from nrsc5_amd import wideband
    raw, rate, fmt, _, _ = _scene("C")
    nominated = wideband.scan(raw, rate, fmt, confirm=False, lib_path=hip_lib)
    print([(round(s.offset_hz / 1e3, 1), round(s.score_db, 1)) for s in nominated])
    assert len(nominated) <= 1 and all(abs(s.offset_hz - 3.0e6) > 150e3 for s in nominated)
    assert wideband.scan(raw, rate, fmt, lib_path=hip_lib) == []


# ---- the CLI without --offsets ------------------------------------------------------------------------------------------------------
def _decodes_truth(log, cap, s, n_frames):
    """every P1 frame decoded with a low BER is a transmitted one, and at least n_frames - 1 of them arrive; same for PIDS"""
    p1 = [v["bits"] for k, v in log if k == "frame" and v["lc"] == 0]
    pids = [v["bits"] for k, v in log if k == "pids"]
    sent_p1 = {f.tobytes() for f in cap.p1[s]}
    sent_pids = {f.tobytes() for f in cap.pids[s]}
    bers = [v["cber"] for k, v in log if k == "ber"]
    good = [f for f, b in zip(p1, bers) if b < 0.02]
    ok_p1 = len(good) >= n_frames - 1 and all(f.tobytes() in sent_p1 for f in good)
    ok_pids = sum(f.tobytes() in sent_pids for f in pids) >= 0.9 * len(pids) and len(pids) >= 16 * (n_frames - 1)
    return ok_p1, ok_pids, len(good), len(pids)


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "nrsc5_amd.wideband"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_gpu_cli_scan_equals_hand_typed_offsets(hip_lib, tmp_path):
    from nrsc5_amd import synth_wideband as sw, wideband
    offs, levels = [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
    st = [sw.Station(offset_hz=o, seed=500 + k, level=a) for k, (o, a) in enumerate(zip(offs, levels))]
    cap = sw.capture(st, 2400000, "cu8", n_frames=2, noise_rms=0.02, seed=3, device=_dev())      # scene A, two frames long
    f = tmp_path / "band.cu8"
    cap.raw.cpu().numpy().tofile(f)
    csv = tmp_path / "band.csv"
    base = [str(f), "--format", "cu8", "--rate", "2400000"]
    out = _cli(base + ["--spectrum", str(csv)]).splitlines()
    found = [l for l in out if l.startswith("found ")]
    syncs = [l for l in out if " SYNC " in l]
    assert len(found) == 3 and out[:3] == found, out[:6]
    bw = 2400000 / 2048
    centres = [float(l.split()[1]) * 1e3 for l in found]
    for c, o in zip(centres, offs):
        assert abs(c - o) <= 1.5 * bw + 50.0                       # the line prints 0.1 kHz
        assert " psmi 1" in found[centres.index(c)]
    assert len(syncs) == 3 and len({l.split(":")[0] for l in syncs}) == 3, syncs
    rows = open(csv).read().splitlines()
    assert rows[0] == "freq_hz,power_db" and len(rows) == 1 + 2048
    assert _cli(base + ["--scan-only"]).splitlines() == found
    # the same decode through the library: every station found decodes the transmitted frames
    stations = wideband.scan(cap.raw, cap.rate, cap.fmt, seconds=1.0, lib_path=hip_lib)
    assert [f"{s.offset_hz / 1e3:+.1f}" for s in stations] == [l.split()[1] for l in found]
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, [s.offset_hz for s in stations], q15_capacity=int(n / 2.4e6 * 744187.5) + 4 * 71280,
                                   lib_path=hip_lib)
    for p in range(0, n, 1 << 22):
        rx.push(cap.raw[2 * p:2 * min(n, p + (1 << 22))])
    for s in range(3):
        ok_p1, ok_pids, n1, n2 = _decodes_truth(rx.logs[s], cap, s, 2)
        assert ok_p1 and ok_pids, (s, n1, n2)
        assert [format_ for format_ in (wideband.format_event(rx, s, k, v) for k, v in rx.logs[s]) if format_ and " SYNC " in format_][0] in syncs
    rx.close()
    # --offsets still prints what it printed before: one SYNC line per station, nothing about a scan
    typed = _cli(base + ["--offsets", "-800e3,0,600e3"]).splitlines()
    assert not any(l.startswith("found ") for l in typed)
    t_syncs = [l for l in typed if " SYNC " in l]
    assert {l.split(":")[0] for l in t_syncs} == {"station 0 (-800.0 kHz)", "station 1 (+0.0 kHz)", "station 2 (+600.0 kHz)"} and len(t_syncs) == 3
