"""`-m "not gpu"`: the wideband channelizer (nrsc5hip_chan_*, nrsc5_amd/csrc/k_channelize.hip) on the CPU-emulated twin, against the
float64 restatement of its definition (tests/chan_model.py).  The twin's "device" memory is host memory, so numpy buffers are passed
by address here -- never to the real library."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import chan_model as cm

RATES_RESPONSE = [(1488375, 1), (2048000, 1), (2400000, 1), (2500000, 1), (3200000, 1), (6000000, 1), (10000000, 1), (20000000, 1),
                  (1488375, 2), (1000000, 1), (1200000, 1), (20000000, 3), (30720000, 1), (40000000, 1), (56000000, 1), (64000000, 1)]


def _rate_id(r):
    return str(r[0]) if r[1] == 1 else f"{r[0]}over{r[1]}"


def _chan(emu_lib, rate, fmt, offsets, gains=None):
    return eng.Channelizer(rate, fmt, offsets, gains=gains, lib_path=emu_lib)


def _raw(fmt: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if fmt == eng.IQ_CU8:
        return np.clip(np.rint(127 + 40 * rng.standard_normal(2 * n)), 0, 255).astype(np.uint8)
    if fmt == eng.IQ_CS16:
        return np.clip(np.rint(3000 * rng.standard_normal(2 * n)), -32768, 32767).astype(np.int16)
    return (0.1 * rng.standard_normal(2 * n)).astype(np.float32)


def _run(ch, raw: np.ndarray, chunks) -> tuple:
    """push raw in the given chunk sizes; -> int16 [K, M, 2] and the per-call output counts checked against outputs_for"""
    n_total = raw.size // 2
    cap = ch.outputs_for(n_total) + 8
    out = np.zeros((ch.nchan, cap, 2), dtype=np.int16)
    pos, got = 0, 0
    for c in chunks:
        c = min(c, n_total - pos)
        if c <= 0:
            break
        want = ch.outputs_for(c)
        seg = np.ascontiguousarray(raw[2 * pos:2 * (pos + c)])
        tmp = np.zeros((ch.nchan, max(want, 1), 2), dtype=np.int16)
        n = ch.process(seg.ctypes.data, c, tmp.ctypes.data, 2 * tmp.shape[1], tmp.shape[1])
        assert n == want
        out[:, got:got + n] = tmp[:, :n]
        got += n
        pos += c
    assert pos == n_total
    return out[:, :got]


def _response_db(tab: np.ndarray, freqs: np.ndarray, fs: float) -> np.ndarray:
    """|H_p(f)| in dB of every phase row p at every frequency, evaluated in blocks of frequencies: at 64 MS/s the stopband grid has
    7400 points and the whole exponent matrix (taps x points) would dominate the CPU suite's memory and time"""
    j = np.arange(tab.shape[1])
    block = max(1, 400000 // tab.shape[1])
    out = [np.abs(tab @ np.exp(-2j * np.pi * np.outer(j, freqs[b:b + block]) / fs)) for b in range(0, freqs.size, block)]
    return 20 * np.log10(np.maximum(np.concatenate(out, axis=1), 1e-30))


@pytest.mark.parametrize("rate", RATES_RESPONSE, ids=[_rate_id(r) for r in RATES_RESPONSE])
def test_prototype_response_every_phase(emu_lib, rate):
    from fractions import Fraction
    ch = _chan(emu_lib, Fraction(*rate), eng.IQ_CS16, [0.0])
    tab = ch.table().astype(np.float64)
    L, T = tab.shape
    assert (L, T) == (ch.phases, ch.taps)
    fs = rate[0] / rate[1]
    step = fs / (16 * T)
    fp = np.arange(0.0, cm.PASS_HZ + step, step)
    fp[-1] = cm.PASS_HZ
    pdb = _response_db(tab, fp, fs)
    assert pdb.shape == (L, fp.size)
    assert np.max(np.abs(pdb)) <= 0.1, np.max(np.abs(pdb))
    # Below 2 * STOP_HZ (about 1.09 MS/s) no stopband frequency lies inside Nyquist: the stopband is what would alias into +-198.4 kHz
    # of the output, STOP_HZ = 744 187.5 - 198.4 k, and nothing within +-Fs/2 of the input reaches that far.  There the passband is
    # the whole check.
    if fs / 2 >= cm.STOP_HZ:
        fstop = np.arange(cm.STOP_HZ, fs / 2 + step, step)
        fstop[-1] = min(fstop[-1], fs / 2)
        sdb = _response_db(tab, fstop, fs)
        assert sdb.shape == (L, fstop.size) and fstop.size >= 1
        assert np.max(sdb) <= -70.0, np.max(sdb)
        print(f"rate {fs:.1f}: passband {np.max(np.abs(pdb)):.4f} dB, stopband {np.max(sdb):.1f} dB, L {L} T {T}")
    ch.close()


def _offsets(fs: float, k: int, seed: int):
    edge = fs / 2 - cm.PASS_HZ
    rng = np.random.default_rng(seed)
    return [edge, -edge] + list(rng.uniform(-edge, edge, k - 2))


@pytest.mark.parametrize("fmt", [eng.IQ_CU8, eng.IQ_CS16, eng.IQ_CF32], ids=["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("rate", [2400000, 3200000])
def test_twin_equals_float64_model(emu_lib, fmt, rate):
    offs = _offsets(rate, 4, seed=rate + fmt)
    ch = _chan(emu_lib, rate, fmt, offs)
    raw = _raw(fmt, 12000, seed=fmt)
    got = _run(ch, raw, [5000, 7000])
    want, y, clips = cm.model(cm.scaled(raw, fmt), rate, 1, offs, None, ch.table())
    assert got.shape == want.shape
    rms = np.sqrt(np.mean(np.abs(y[:, y.shape[1] // 4:]) ** 2, axis=1))
    assert np.all(rms > 200) and np.all(rms < 5000), rms
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1, diff.max()
    assert np.mean(diff != 0) <= 0.01, np.mean(diff != 0)
    assert np.array_equal(ch.clip_counts(), clips)
    ch.close()


def test_rate_edge_table_covers_every_kernel_configuration(emu_lib):
    """cm.RATE_EDGE_CASES is only worth its name while it reaches every configuration of the kernel: the tiles of 256, 64 and 32
    outputs (32: a block of 64 work-items, half of them without an output), P/Q = 1, the phase count clamped to 4096, a fractional
    rate, and taps in the hundreds.  Taps and phases come from the library, so a change of the design constants shows here."""
    seen = []
    for rate in cm.RATE_EDGE_CASES:
        ch = _chan(emu_lib, rate, eng.IQ_CS16, [0.0])
        T, L = ch.taps, ch.phases
        ch.close()
        P, Q = cm.ratio(rate.numerator, rate.denominator)
        mt, span = cm.tile(P, Q, T)
        assert span <= cm.SPAN_MAX and mt >= 32                  # the floor of 16 is out of reach below 64 MS/s
        for k in (1, 11):
            n, chunks = cm.case_size(rate, T, k)
            assert sum(chunks) == n and min(chunks) < T
            M = cm.outputs_total(n, P, Q, T)
            assert M >= 3.5 * mt and cm.outputs_total(chunks[0], P, Q, T) % mt != 0
        print(f"rate {float(rate):.1f}: P/Q {P}/{Q} T {T} L {L} mt {mt} span {span} n {n} M {M}")
        seen.append((rate, P, Q, T, L, mt, span))
    assert {s[5] for s in seen} == {256, 64, 32}
    assert any(s[1] == s[2] == 1 for s in seen)
    assert any(s[4] == 4096 for s in seen) and any(s[4] < 64 for s in seen)
    assert any(s[0].denominator != 1 and s[0] != cm.OUT_RATE for s in seen)
    assert any(s[3] > 400 and s[5] == 32 for s in seen)
    assert max(s[6] for s in seen) > 0.9 * cm.SPAN_MAX          # a tile that nearly fills the LDS


@pytest.mark.parametrize("case", cm.edge_case_params(), ids=cm.edge_case_id)
def test_twin_equals_float64_model_over_the_rate_range(emu_lib, case):
    """Every kernel configuration the rate selects, with odd channel counts; the input level is chosen per rate so that the model's
    output rms lies in 800..2500 LSB, where the 2.4 / 10 / 20 MS/s cases sit.  Measured on the twin: largest difference 1 LSB, at most
    0.074 % of the values differing, clip counts equal at every case."""
    rate, fmt, k = case
    fs = float(rate)
    seed = rate.numerator % 997 + 10 * fmt + k
    offs = _offsets(fs, max(k, 2), seed)[:k]
    ch = _chan(emu_lib, rate, fmt, offs)
    n, chunks = cm.case_size(rate, ch.taps, k)
    raw = cm.raw_noise(fmt, n, seed, cm.level(rate))
    got = _run(ch, raw, chunks)
    want, y, clips = cm.model(cm.scaled(raw, fmt), rate.numerator, rate.denominator, offs, None, ch.table())
    cm.assert_equals_model(got, ch.clip_counts(), want, clips, y, rms_range=(800, 2500))
    ch.close()


def test_chunking_is_byte_identical_with_more_taps_than_samples(emu_lib):
    """64 MS/s: 926 taps, tiles of 32 outputs.  Chunks of 7 and of T - 1 samples never hold one output's whole support, so every output
    is summed from the history and from several pushes; one channel clips some of its outputs."""
    rate, fmt, k, n = cm.RATE_EDGE_CASES[-1], eng.IQ_CS16, 11, 30000
    offs = _offsets(float(rate), k, seed=64)
    gains = [1.0] * (k - 1) + [cm.CLIP_GAIN]
    raw = cm.raw_noise(fmt, n, 64, cm.level(rate))
    rng = np.random.default_rng(64)
    ref = None
    for plan in ("whole", "sevens", "taps-1", "random"):
        ch = _chan(emu_lib, rate, fmt, offs, gains)
        T = ch.taps
        chunks = {"whole": [n], "sevens": [7] * (n // 7 + 1), "taps-1": [T - 1] * (n // (T - 1) + 1),
                  "random": list(rng.integers(1, 3001, 200))}[plan]
        assert sum(chunks) >= n and T > 900
        out, clips = _run(ch, raw, chunks), ch.clip_counts()
        if ref is None:
            ref = (out, clips)
            assert 0 < clips[k - 1] < out.shape[1] and not clips[:k - 1].any(), (clips, out.shape)
            want, _, want_clips = cm.model(cm.scaled(raw, fmt), rate.numerator, rate.denominator, offs, gains, ch.table())
            cm.assert_equals_model(out, clips, want, want_clips)
        else:
            assert out.tobytes() == ref[0].tobytes(), plan
            assert np.array_equal(clips, ref[1]), plan
        ch.close()


def test_chunking_is_byte_identical(emu_lib):
    rate, fmt = 2400000, eng.IQ_CS16
    offs = _offsets(rate, 3, seed=5)
    raw = _raw(fmt, 9000, seed=11)
    gains = [1.0, 1.0, 40.0]                                   # the third channel clips
    rng = np.random.default_rng(3)
    results = []
    for chunks in ([9000], [7] * 1300, [4093] * 3, list(rng.integers(1, 900, 100)), [1] * 9000):
        ch = _chan(emu_lib, rate, fmt, offs, gains)
        results.append((_run(ch, raw, chunks), ch.clip_counts()))
        ch.close()
    assert results[0][1][2] > 0 and results[0][1][0] == 0
    for out, clips in results[1:]:
        assert out.tobytes() == results[0][0].tobytes()
        assert np.array_equal(clips, results[0][1])


def test_reset_equals_fresh_object(emu_lib):
    rate, fmt = 3200000, eng.IQ_CU8
    offs = _offsets(rate, 2, seed=8)
    raw = _raw(fmt, 6000, seed=2)
    ch = _chan(emu_lib, rate, fmt, offs, [30.0, 1.0])
    first = _run(ch, raw, [2500, 3500])
    c1 = ch.clip_counts()
    ch.reset()
    assert ch.outputs_for(6000) == first.shape[1]
    second = _run(ch, raw, [6000])
    assert second.tobytes() == first.tobytes() and np.array_equal(ch.clip_counts(), c1)
    ch.close()


def test_realised_offsets(emu_lib):
    for rate in (2048000, (20000000, 3), 10000000):
        num, den = rate if isinstance(rate, tuple) else (rate, 1)
        fs = num / den
        offs = _offsets(fs, 8, seed=num)
        from fractions import Fraction
        ch = _chan(emu_lib, Fraction(num, den), eng.IQ_CS16, offs)
        assert np.all(np.abs(ch.realised - np.asarray(offs)) <= fs / 2 ** 33), ch.realised - offs
        ch.close()


def test_rejected_arguments(emu_lib):
    def rejects(rate, fmt, offs, code=eng.EINVAL):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            _chan(emu_lib, rate, fmt, offs)
        assert ei.value.code == code
    rejects(744187, eng.IQ_CS16, [0.0])                         # below 744 187.5
    rejects(64000001, eng.IQ_CS16, [0.0])                       # above 64 MS/s
    rejects(2400000, eng.IQ_CS16, [1200000 - 198500 + 1.0])     # |f| > Fs/2 - 198.5 kHz
    rejects(2400000, eng.IQ_CS16, [-(1200000 - 198500 + 1.0)])
    rejects(2400000, eng.IQ_CS16, np.zeros(513))                 # K > 512
    rejects(2400000, 3, [0.0])                                  # bad format
    with pytest.raises(eng.Nrsc5HipError) as ei:
        _chan(emu_lib, 2400000, eng.IQ_CS16, np.zeros(0))       # K = 0
    assert ei.value.code == eng.EINVAL
    ch = _chan(emu_lib, 744187.5, eng.IQ_CS16, [1000.0, -173000.0])   # the edges of the range are accepted
    ch.close()
    ch = _chan(emu_lib, 64000000, eng.IQ_CS16, [31.8e6 - 1.0])
    ch.close()

    # EOVERFLOW leaves the object untouched: the same push with room gives what a fresh object gives
    rate, fmt = 2400000, eng.IQ_CS16
    raw = _raw(fmt, 4000, seed=9)
    ch = _chan(emu_lib, rate, fmt, [0.0, 300e3])
    want = ch.outputs_for(4000)
    small = np.zeros((2, want - 1, 2), dtype=np.int16)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        ch.process(raw.ctypes.data, 4000, small.ctypes.data, 2 * (want - 1), want - 1)
    assert ei.value.code == eng.EOVERFLOW
    assert ch.outputs_for(4000) == want
    with pytest.raises(eng.Nrsc5HipError) as ei:                # stride shorter than the capacity
        ch.process(raw.ctypes.data, 4000, small.ctypes.data, want, want)
    assert ei.value.code == eng.EINVAL
    got = _run(ch, raw, [4000])
    fresh = _chan(emu_lib, rate, fmt, [0.0, 300e3])
    assert got.tobytes() == _run(fresh, raw, [4000]).tobytes()
    ch.close()
    fresh.close()


def test_feed_refused_by_the_engine_leaves_the_channelizer_untouched(emu_lib):
    rate, fmt = 2400000, eng.IQ_CS16
    raw = _raw(fmt, 4000, seed=12)
    E = eng.Engine(max_streams=2, q15_capacity=2 * 71280, record_capacity=64, p1_slots=2, lib_path=emu_lib)
    ch = _chan(emu_lib, rate, fmt, [0.0, 300e3], [50.0, 1.0])
    want = ch.outputs_for(4000)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        ch.feed(E, [0, 7], raw.ctypes.data, 4000)                # stream 7 does not exist
    assert ei.value.code == eng.EINVAL and "stream" in str(ei.value)
    assert ch.outputs_for(4000) == want and not ch.clip_counts().any()
    got = _run(ch, raw, [4000])
    fresh = _chan(emu_lib, rate, fmt, [0.0, 300e3], [50.0, 1.0])
    assert got.tobytes() == _run(fresh, raw, [4000]).tobytes()
    assert np.array_equal(ch.clip_counts(), fresh.clip_counts()) and ch.clip_counts()[0] > 0
    ch.close(); fresh.close(); E.close()


def test_outputs_for_reports_its_error(emu_lib):
    ch = _chan(emu_lib, 2400000, eng.IQ_CS16, [0.0])
    with pytest.raises(eng.Nrsc5HipError) as ei:
        ch.outputs_for(-1)
    assert "negative" in str(ei.value)
    ch.close()
