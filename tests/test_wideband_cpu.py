"""`-m "not gpu"`: the wideband channelizer (nrsc5hip_chan_*, nrsc5_amd/csrc/k_channelize.hip) on the CPU-emulated twin, against the
float64 restatement of its definition (tests/chan_model.py).  The twin's "device" memory is host memory, so numpy buffers are passed
by address here -- never to the real library."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import chan_model as cm

RATES_RESPONSE = [(1488375, 1), (2048000, 1), (2400000, 1), (2500000, 1), (3200000, 1), (6000000, 1), (10000000, 1), (20000000, 1)]


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


@pytest.mark.parametrize("rate", RATES_RESPONSE, ids=[str(r[0]) for r in RATES_RESPONSE])
def test_prototype_response_every_phase(emu_lib, rate):
    ch = _chan(emu_lib, rate[0], eng.IQ_CS16, [0.0])
    tab = ch.table().astype(np.float64)
    L, T = tab.shape
    assert (L, T) == (ch.phases, ch.taps)
    fs = rate[0] / rate[1]
    step = fs / (16 * T)
    fp = np.arange(0.0, cm.PASS_HZ + step, step)
    fp[-1] = cm.PASS_HZ
    fstop = np.arange(cm.STOP_HZ, fs / 2 + step, step)
    fstop[-1] = min(fstop[-1], fs / 2)
    j = np.arange(T)
    hp = np.abs(tab @ np.exp(-2j * np.pi * np.outer(j, fp) / fs))
    hs = np.abs(tab @ np.exp(-2j * np.pi * np.outer(j, fstop) / fs))
    pdb, sdb = 20 * np.log10(hp), 20 * np.log10(np.maximum(hs, 1e-30))
    assert np.max(np.abs(pdb)) <= 0.1, np.max(np.abs(pdb))
    assert np.max(sdb) <= -70.0, np.max(sdb)
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
