"""GPU: the wideband channelizer (nrsc5hip_chan_*) on the MI355X -- against the float64 restatement of its definition
(tests/chan_model.py), byte-identical across chunkings, fed into the batch engine exactly as the outputs appended by hand, and the
error floor of the prototype (stopband tone, multi-station capture against the ideal float64 channelizer)."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import chan_model as cm

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _raw(fmt: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if fmt == eng.IQ_CU8:
        return np.clip(np.rint(127 + 40 * rng.standard_normal(2 * n)), 0, 255).astype(np.uint8)
    if fmt == eng.IQ_CS16:
        return np.clip(np.rint(3000 * rng.standard_normal(2 * n)), -32768, 32767).astype(np.int16)
    return (0.1 * rng.standard_normal(2 * n)).astype(np.float32)


def _offsets(fs: float, k: int, seed: int):
    edge = fs / 2 - cm.PASS_HZ
    rng = np.random.default_rng(seed)
    return [edge, -edge] + list(rng.uniform(-edge, edge, k - 2))


def _push(ch, x, chunks):
    """torch device tensor pushed in chunks (samples); -> numpy int16 [K, M, 2]"""
    import torch
    outs, pos, n = [], 0, x.numel() // 2
    for c in chunks:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        want = ch.outputs_for(c)
        o = ch.process_tensor(x[2 * pos:2 * (pos + c)])
        assert o.shape[1] == want
        outs.append(o)
        pos += c
    assert pos == n
    return torch.cat(outs, dim=1).cpu().numpy()


def _check_model(rate, fmt, k, n, seed, hip_lib):
    import torch
    offs = _offsets(rate, k, seed)
    raw = _raw(fmt, n, seed)
    ch = eng.Channelizer(rate, fmt, offs, lib_path=hip_lib)
    got = _push(ch, torch.from_numpy(raw).to(_dev()), [n // 3, n - n // 3])
    want, y, clips = cm.model(cm.scaled(raw, fmt), rate, 1, offs, None, ch.table())
    assert got.shape == want.shape
    rms = np.sqrt(np.mean(np.abs(y[:, y.shape[1] // 4:]) ** 2, axis=1))
    assert np.all(rms > 200) and np.all(rms < 5000), rms
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1, diff.max()
    assert np.mean(diff != 0) <= 0.01, np.mean(diff != 0)
    assert np.array_equal(ch.clip_counts(), clips)
    ch.close()


@pytest.mark.parametrize("fmt", [eng.IQ_CU8, eng.IQ_CS16, eng.IQ_CF32], ids=["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("rate", [2400000, 10000000])
def test_gpu_device_equals_float64_model(hip_lib, fmt, rate):
    _check_model(rate, fmt, 16, 60000 if rate < 5e6 else 200000, seed=rate % 997 + fmt, hip_lib=hip_lib)


def test_gpu_device_equals_float64_model_20msps_64_channels(hip_lib):
    _check_model(20000000, eng.IQ_CS16, 64, 200000, seed=64, hip_lib=hip_lib)


@pytest.mark.parametrize("case", cm.edge_case_params(), ids=cm.edge_case_id)
def test_gpu_device_equals_float64_model_over_the_rate_range(hip_lib, case):
    """Every kernel configuration the rate selects (tests/chan_model.py: RATE_EDGE_CASES; tiles of 256, 64 and 32 outputs, the block of
    64 work-items over a tile of 32, P/Q = 1, 4096 phases, a fractional rate, up to 926 taps) with odd channel counts, pushed in chunks
    that split a tile and include one shorter than the taps.  The input level is set per rate so that the model's output rms lies in
    800..2500 LSB, where the 2.4 / 10 / 20 MS/s cases sit: the share of values the fast sincos may move is then comparable across
    the rates.  Measured on the device (profiles/wideband_edge_cases.txt): largest difference 1 LSB, at most 0.075 % of the values
    differing."""
    import torch
    rate, fmt, k = case
    seed = rate.numerator % 997 + 10 * fmt + k
    offs = _offsets(float(rate), max(k, 2), seed)[:k]
    ch = eng.Channelizer(rate, fmt, offs, lib_path=hip_lib)
    n, chunks = cm.case_size(rate, ch.taps, k)
    raw = cm.raw_noise(fmt, n, seed, cm.level(rate))
    got = _push(ch, torch.from_numpy(raw).to(_dev()), chunks)
    want, y, clips = cm.model(cm.scaled(raw, fmt), rate.numerator, rate.denominator, offs, None, ch.table())
    print(f"chan {cm.edge_case_id(case)} T {ch.taps} L {ch.phases} n {n} M {want.shape[1]}: ", end="")
    cm.assert_equals_model(got, ch.clip_counts(), want, clips, y, rms_range=(800, 2500))
    ch.close()


def test_gpu_chunking_is_byte_identical_with_more_taps_than_samples(hip_lib):
    """64 MS/s: 926 taps, tiles of 32 outputs under a block of 64.  Chunks of 7 and of T - 1 samples never hold one output's whole
    support, so every output is summed from the history and from several pushes; one channel clips some of its outputs (measured: 53
    of 344, as the model; 0.11 % of the values differing from it by 1 LSB)."""
    import torch
    rate, fmt, k, n = cm.RATE_EDGE_CASES[-1], eng.IQ_CS16, 11, 30000
    offs = _offsets(float(rate), k, seed=64)
    gains = [1.0] * (k - 1) + [cm.CLIP_GAIN]
    raw = cm.raw_noise(fmt, n, 64, cm.level(rate))
    x = torch.from_numpy(raw).to(_dev())
    rng = np.random.default_rng(64)
    ref = None
    for plan in ("whole", "sevens", "taps-1", "random"):
        ch = eng.Channelizer(rate, fmt, offs, gains=gains, lib_path=hip_lib)
        T = ch.taps
        chunks = {"whole": [n], "sevens": [7] * (n // 7 + 1), "taps-1": [T - 1] * (n // (T - 1) + 1),
                  "random": list(rng.integers(1, 3001, 200))}[plan]
        assert sum(chunks) >= n and T > 900
        out, clips = _push(ch, x, chunks), ch.clip_counts()
        if ref is None:
            ref = (out, clips)
            assert 0 < clips[k - 1] < out.shape[1] and not clips[:k - 1].any(), (clips, out.shape)
            want, _, want_clips = cm.model(cm.scaled(raw, fmt), rate.numerator, rate.denominator, offs, gains, ch.table())
            print("chan 64000000-cs16-K11 one channel clipping, one push: ", end="")
            cm.assert_equals_model(out, clips, want, want_clips)
        else:
            assert out.tobytes() == ref[0].tobytes(), plan
            assert np.array_equal(clips, ref[1]), plan
        ch.close()


def test_gpu_chunking_is_byte_identical(hip_lib):
    import torch
    rate, fmt, n = 10000000, eng.IQ_CS16, 150000
    offs = _offsets(rate, 12, seed=1)
    x = torch.from_numpy(_raw(fmt, n, seed=4)).to(_dev())
    gains = [1.0] * 11 + [30.0]
    rng = np.random.default_rng(7)
    ref, ref_clips = None, None
    for chunks in ([n], [7] * (n // 7 + 1), [4093] * (n // 4093 + 1), list(rng.integers(1, 20000, 200))):
        ch = eng.Channelizer(rate, fmt, offs, gains=gains, lib_path=hip_lib)
        out = _push(ch, x, chunks)
        clips = ch.clip_counts()
        ch.close()
        if ref is None:
            ref, ref_clips = out, clips
            assert clips[11] > 0
        else:
            assert out.tobytes() == ref.tobytes()
            assert np.array_equal(clips, ref_clips)


def test_gpu_feed_equals_process_and_batch_append(hip_lib):
    """nrsc5hip_chan_feed in random chunks, records drained after every feed, == the whole capture channelized, appended with
    nrsc5hip_batch_append_cs16 and decoded in one batch"""
    import torch
    from nrsc5_amd import synth
    cap = synth.fm_mp1_capture(0, seed=5, cfo_hz=-140.0, offset=1701, snr_db=22.0, n_blocks=40)
    iq = np.ascontiguousarray(cap.iq, dtype=np.uint8)
    n = iq.size // 2
    offs = [0.0, 2000.0]
    x = torch.from_numpy(iq).to(_dev())
    torch.cuda.synchronize()

    def engine():
        return eng.Engine(max_streams=2, q15_capacity=n // 2 + 4 * 71280, record_capacity=512, p1_slots=8, p1_async=True,
                          l2_feedback=True, lib_path=hip_lib)

    ch = eng.Channelizer(1488375, eng.IQ_CU8, offs, lib_path=hip_lib)
    y = ch.process_tensor(x)
    m = y.shape[1]
    E = engine()
    E.batch_append_cs16(y.data_ptr(), 2 * m, [2 * m, 2 * m], stream_ids=[0, 1])
    E.batch_process(2, stream_ids=[0, 1])
    want = [E.drain(s).tobytes() for s in (0, 1)]
    E.close()
    ch.close()

    ch = eng.Channelizer(1488375, eng.IQ_CU8, offs, lib_path=hip_lib)
    E = engine()
    got = [b"", b""]
    rng = np.random.default_rng(13)
    pos = 0
    while pos < n:
        c = min(int(rng.integers(1000, 300000)), n - pos)
        ch.feed(E, [0, 1], x[2 * pos:].data_ptr(), c)
        E.batch_process(2, stream_ids=[0, 1])
        for s in (0, 1):
            got[s] += E.drain(s).tobytes()
        pos += c
    E.close()
    ch.close()
    assert len(want[0]) > 0 and got == want
    recs = np.frombuffer(want[0], dtype=eng.RECORD_DTYPE)
    assert np.any(recs["flags"] & eng.REC_TO_FINE)


def test_gpu_stopband_tone_70db_below_passband_tone(hip_lib):
    import torch
    rate, n = 10000000, 200000
    t = np.arange(n)
    for f_stop in (545.8e3, 700e3, 2.3e6):
        rows = []
        for f in (f_stop, 50e3):
            z = 0.5 * np.exp(2j * np.pi * f * t / rate)              # -6 dBFS
            raw = np.stack([z.real, z.imag], axis=-1).reshape(-1).astype(np.float32)
            ch = eng.Channelizer(rate, eng.IQ_CF32, [0.0], lib_path=hip_lib)
            y = _push(ch, torch.from_numpy(raw).to(_dev()), [n])[0].astype(np.float64)
            ch.close()
            y = y[y.shape[0] // 4:]
            rows.append(np.mean(y[:, 0] ** 2 + y[:, 1] ** 2))
        ratio_db = 10 * np.log10(max(rows[0], 1e-30) / rows[1])
        assert ratio_db <= -70.0, (f_stop, ratio_db)


def test_gpu_multi_station_capture_against_ideal_channelizer(hip_lib):
    import torch
    rate, n = 10000000, 120000
    rng = np.random.default_rng(21)
    offs = [-3.2e6, -1.4e6, -1.2e6, 0.0, 2.6e6, 4.7e6]
    levels = [1.0, 0.3, 1.0, 0.6, 0.1, 0.8]
    f = np.fft.fftfreq(n, 1 / rate)
    x = np.zeros(n, dtype=np.complex128)
    for o, a in zip(offs, levels):
        s = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
        s[np.abs(f) > 190e3] = 0
        st = np.fft.ifft(s)
        x += a * st / np.sqrt(np.mean(np.abs(st) ** 2)) * np.exp(2j * np.pi * o * np.arange(n) / rate)
    x *= 4000 / np.sqrt(np.mean(np.abs(x) ** 2))
    raw = np.clip(np.rint(np.stack([x.real, x.imag], axis=-1).reshape(-1)), -32768, 32767).astype(np.int16)
    xs = cm.scaled(raw, eng.IQ_CS16)
    T = eng.Channelizer(rate, eng.IQ_CS16, offs, lib_path=hip_lib).taps
    M = cm.outputs_total(n, *cm.ratio(rate, 1), T)
    unit = cm.ideal(xs, rate, 1, offs, None, T, M)
    gains = [3000.0 / np.sqrt(np.mean(np.abs(u[T:]) ** 2)) for u in unit]      # each output ~3000 LSB rms
    ch = eng.Channelizer(rate, eng.IQ_CS16, offs, gains=gains, lib_path=hip_lib)
    got = _push(ch, torch.from_numpy(raw).to(_dev()), [n // 2, n - n // 2])
    ch.close()
    assert got.shape[1] == M
    want = unit * np.asarray(gains)[:, None]
    g = got[..., 0] + 1j * got[..., 1]
    skip = T                                                     # past the start-up transient of the zero history
    for k in range(len(offs)):
        e = g[k, skip:] - want[k, skip:]
        rms = np.sqrt(np.mean(np.abs(want[k, skip:]) ** 2))
        assert 1500 < rms < 6000, rms
        err_db = 10 * np.log10(np.mean(np.abs(e) ** 2) / rms ** 2)
        assert err_db <= -70.0, (k, err_db)


# ---- end to end: synthetic band captures (nrsc5_amd/synth_wideband.py) through nrsc5_amd/wideband.py ----------------------------
def _truth_frames(log):
    p1 = [v["bits"] for k, v in log if k == "frame" and v["lc"] == 0]
    pids = [v["bits"] for k, v in log if k == "pids"]
    return p1, pids


def _decodes_truth(log, cap, s, n_frames):
    """every P1 frame decoded with a low BER is a transmitted one, and at least n_frames - 1 of them arrive; same for PIDS"""
    p1, pids = _truth_frames(log)
    sent_p1 = {f.tobytes() for f in cap.p1[s]}
    sent_pids = {f.tobytes() for f in cap.pids[s]}
    bers = [v["cber"] for k, v in log if k == "ber"]
    good = [f for f, b in zip(p1, bers) if b < 0.02]
    ok_p1 = len(good) >= n_frames - 1 and all(f.tobytes() in sent_p1 for f in good)
    ok_pids = sum(f.tobytes() in sent_pids for f in pids) >= 0.9 * len(pids) and len(pids) >= 16 * (n_frames - 1)
    return ok_p1, ok_pids, len(good), len(pids)


def _receive(cap, offsets, chunk, hip_lib, gains=None):
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offsets, gains=gains, q15_capacity=q15, lib_path=hip_lib)
    for p in range(0, n, chunk):
        rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
    return rx


def test_gpu_end_to_end_10msps_cs16_8_stations_equal_reference(hip_lib, reflib):
    import argparse
    import bench
    from nrsc5_amd import channel, synth_wideband as sw
    from tests.test_gpu_batch256 import HARD_CLASSES
    n_frames = 3
    offs = [-4.6e6, -3.0e6, -1.8e6, -1.6e6, 0.4e6, 1.2e6, 2.8e6, 4.4e6]      # -1.8 / -1.6 MHz: 200 kHz apart, 20 dB apart
    levels = [1.0, 0.7, 1.0, 0.1, 0.5, 0.8, 1.0, 0.6]
    rng = np.random.default_rng(808)
    st = [sw.Station(offset_hz=o, seed=300 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)),
                     chan=channel.Impairments(host_db=20.0) if k == 5 else None)
          for k, (o, a) in enumerate(zip(offs, levels))]
    cap = sw.capture(st, 10000000, "cs16", n_frames=n_frames, noise_rms=0.05, rms_total=6000.0, seed=8, device=_dev())
    rx = _receive(cap, offs, 3_000_000, hip_lib)
    # the reference runs on the very cs16 bytes the engine decoded (the channelizer's output, copied back)
    ch = eng.Channelizer(cap.rate, eng.IQ_CS16, offs, lib_path=hip_lib)
    y = ch.process_tensor(cap.raw).cpu().numpy()
    ch.close()
    S = len(offs)
    recs = [rx.station_records(s) for s in range(S)]
    counts = np.array([len(r) for r in recs])
    R = np.zeros((S, max(counts)), dtype=eng.RECORD_DTYPE)
    for s in range(S):
        R[s, :counts[s]] = recs[s]
    W = argparse.Namespace()
    W.eng, W.name, W.my_streams, W.checkable = eng, "wideband", list(range(S)), list(range(S))
    W.args = argparse.Namespace(oracle_streams=-1, oracle_lost_max=S, parity_processes=S)
    W.stream_iq = lambda k: np.ascontiguousarray(y[k].reshape(-1))
    W.impaired = lambda k: k == 5
    n_fail0 = len(bench.FAILURES)
    out = bench.reference_equality(W, R, counts, [None] * S, lambda k, r, fr: rx.logs[k], am=False)
    del bench.FAILURES[n_fail0:]
    print({k: v for k, v in out.items() if k not in ("compared", "checker")})
    assert out["kind"] == "reference" and out["streams_compared"] == S
    classes = out["streams_failing_by_class"]
    assert not any(c in classes for c in HARD_CLASSES), (classes, out["first_diffs"])
    assert S - out["streams_equal_under_the_strict_rule"] <= 1, (classes, out["first_diffs"])
    for s in range(S):
        assert any(k == "sync" for k, _ in rx.logs[s]), s
        if cap.snr_db[s] >= 15:
            ok_p1, ok_pids, n1, n2 = _decodes_truth(rx.logs[s], cap, s, n_frames)
            assert ok_p1 and ok_pids, (s, cap.snr_db[s], n1, n2)
    rx.close()


@pytest.mark.parametrize("case", ["rtlsdr_2.4M_cu8", "20M_cf32"])
def test_gpu_end_to_end_small_captures(hip_lib, case):
    from nrsc5_amd import synth_wideband as sw
    if case == "rtlsdr_2.4M_cu8":
        rate, fmt, offs, levels = 2400000, "cu8", [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
    else:
        rate, fmt, offs, levels = 20000000, "cf32", [-9.0e6, -2.2e6, 3.4e6, 9.2e6], [1.0, 0.5, 0.8, 0.7]
    rng = np.random.default_rng(rate)
    st = [sw.Station(offset_hz=o, seed=500 + k, cfo_hz=float(rng.uniform(-3000, 3000)), level=a, timing=int(rng.integers(0, 4320)))
          for k, (o, a) in enumerate(zip(offs, levels))]
    cap = sw.capture(st, rate, fmt, n_frames=2, noise_rms=0.02, seed=3, device=_dev())
    rx = _receive(cap, offs, 1_000_003, hip_lib)
    for s in range(len(offs)):
        assert sum(k == "sync" for k, _ in rx.logs[s]) >= 1, s
        assert cap.snr_db[s] >= 15
        ok_p1, ok_pids, n1, n2 = _decodes_truth(rx.logs[s], cap, s, 2)
        assert ok_p1 and ok_pids, (s, n1, n2)
    rx.close()


def test_gpu_cli_prints_one_sync_per_station(tmp_path):
    import subprocess
    import sys
    from nrsc5_amd import synth_wideband as sw
    offs = [-400e3, 600e3]
    st = [sw.Station(offset_hz=o, seed=700 + k, cfo_hz=150.0 * (k + 1), timing=900 * k) for k, o in enumerate(offs)]
    cap = sw.capture(st, 2048000, "cs16", n_frames=1, noise_rms=0.02, seed=5, device=_dev())
    f = tmp_path / "band.cs16"
    cap.raw.cpu().numpy().tofile(f)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "nrsc5_amd.wideband", str(f), "--format", "cs16", "--rate", "2048000",
                        "--offsets", ",".join(str(o) for o in offs)], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    syncs = [l for l in r.stdout.splitlines() if " SYNC " in l]
    assert len(syncs) == 2 and syncs[0] != syncs[1], r.stdout
    assert {l.split(":")[0] for l in syncs} == {"station 0 (-400.0 kHz)", "station 1 (+600.0 kHz)"}
