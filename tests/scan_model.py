"""float64 restatement of the band scan's definition (include/nrsc5hip.h, nrsc5hip_scan_*) for the tests: the Welch power spectrum
(periodic Hann, 50 % overlap, segments at absolute sample indices) and the sideband detector's rule, plus the synthetic scenes the
detector is checked on."""
from __future__ import annotations

import numpy as np

from tests.chan_model import scaled  # noqa: F401  (the same input scaling as the channelizer)

CARRIER_HZ = 1488375.0 / 4096.0
SB_LO_HZ, SB_HI_HZ = 356 * CARRIER_HZ, 546 * CARRIER_HZ
EDGE_HZ = 198.5e3
FLOOR_QUANTILE = 0.2


def default_nfft(fs: float) -> int:
    n = 512
    while n < 8192 and n < fs / 2000.0:
        n *= 2
    return n


def segments(n: int, nfft: int) -> int:
    return 0 if n < nfft else (n - nfft) // (nfft // 2) + 1


RUN_MAX, ROWS_TARGET = 64, 1024

# Even log2(nfft): the transform is radix-4 passes alone, no radix-2 pre-pass.  (rate, the nfft it defaults to); 4096 is the default
# of every rate in (4.096 M, 8.192 M] and needs more than 64 KiB of LDS.
EVEN_NFFT_CASES = [(1500000, 1024), (6000000, 4096)]

# One push of so many segments that a workgroup sums a run of them in registers (run_rows()): name -> (nfft, n, fmt, chunks,
# run, rows, segments in the last row -- of the largest push).  "rows-over-target": the run clamped to RUN_MAX with more than ROWS_TARGET rows, 72 MB of input.
MANY_SEGMENT_CASES = {
    "run3-cs16": (512, 512 + 256 * 2100 + 99, 1, None, 3, 701, 1),
    "run3-cu8-grow": (512, 512 + 256 * 2100 + 99, 0, [1000], 3, 700, 2),       # the partial-sum rows grow between the two pushes
    "run2-nfft1024": (1024, 1024 + 512 * 1500 + 5, 1, None, 2, 751, 1),
    "rows-over-target": (512, 512 + 256 * 70000 + 11, 1, None, RUN_MAX, 1094, 49),
}


def many_segment_pushes(name: str):
    """-> (nfft, n, fmt, chunk plan); asserts that the case's largest push launches what the table says"""
    nfft, n, fmt, first, run, rows, last = MANY_SEGMENT_CASES[name]
    chunks = (first or []) + [n - sum(first or [])]
    nseg = segments(n, nfft) - segments(n - chunks[-1], nfft)
    assert run_rows(nseg) == (run, rows, last) and run > 1 and last < run
    return nfft, n, fmt, chunks


def run_rows(nseg: int):
    """the launch rule of nrsc5hip_scan_push -> (segments per workgroup, workgroups = rows of partial sums, segments in the last row)"""
    run = min(-(-nseg // ROWS_TARGET), RUN_MAX)
    rows = -(-nseg // run)
    return run, rows, nseg - (rows - 1) * run


def psd(x: np.ndarray, nfft: int, max_segments: int | None = None) -> np.ndarray:
    """x: complex128 in the library's scale -> PSD[nfft], bin i at (i - nfft/2) * fs / nfft"""
    S = segments(x.size, nfft)
    if max_segments is not None:
        S = min(S, max_segments)
    assert S >= 1
    H = nfft // 2
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)
    acc = np.zeros(nfft)
    for s0 in range(0, S, 256):
        idx = (np.arange(s0, min(S, s0 + 256)) * H)[:, None] + np.arange(nfft)[None, :]
        X = np.fft.fft(x[idx] * w[None, :], axis=1)
        acc += np.sum(X.real ** 2 + X.imag ** 2, axis=0)
    return np.fft.fftshift(acc) / (S * np.sum(w * w))


def detect(p: np.ndarray, fs: float, threshold_db: float = 6.0, min_separation_hz: float = 100e3) -> list:
    """the detector's rule -> [{"bin", "offset_hz", "score_db", "lower_db", "upper_db", "floor_db"}, ...], highest score first"""
    nfft = p.size
    bw = fs / nfft
    floor_p = np.sort(p)[int(FLOOR_QUANTILE * (nfft - 1))]
    if not floor_p > 0:
        return []
    pre = np.concatenate([[0.0], np.cumsum(p)])
    pp = np.concatenate([p, [0.0]])

    def integral(f):
        x = np.clip(f / bw + nfft // 2 + 0.5, 0, nfft)
        k = np.floor(x).astype(np.int64)
        return pre[k] + (x - k) * pp[k], x

    def mean(f0, f1):
        (i0, x0), (i1, x1) = integral(f0), integral(f1)
        with np.errstate(divide="ignore", invalid="ignore"):        # centres beyond the edge rule may have an empty window
            return (i1 - i0) / (x1 - x0)

    c = (np.arange(nfft) - nfft // 2) * bw
    ok = np.abs(c) <= fs / 2 - EDGE_HZ
    quarter = (SB_HI_HZ - SB_LO_HZ) / 4
    least = np.full(nfft, np.inf)
    for k in range(4):
        lo, hi = SB_LO_HZ + k * quarter, SB_LO_HZ + (k + 1) * quarter
        least = np.minimum(least, np.minimum(mean(c - hi, c - lo), mean(c + lo, c + hi)))
    with np.errstate(divide="ignore", invalid="ignore"):
        score = 10 * np.log10(least / floor_p)
    cand = [i for i in range(nfft) if ok[i] and np.isfinite(score[i]) and score[i] >= threshold_db]
    cand.sort(key=lambda i: (-score[i], i))
    picks = []
    for i in cand:
        if any(abs(c[i] - q["offset_hz"]) <= min_separation_hz for q in picks):
            continue
        picks.append({"bin": i, "offset_hz": float(c[i]), "score_db": float(score[i]),
                      "lower_db": float(10 * np.log10(mean(c[i:i + 1] - SB_HI_HZ, c[i:i + 1] - SB_LO_HZ)[0] / floor_p)),
                      "upper_db": float(10 * np.log10(mean(c[i:i + 1] + SB_LO_HZ, c[i:i + 1] + SB_HI_HZ)[0] / floor_p)),
                      "floor_db": float(10 * np.log10(floor_p))})
    return picks


def noise_plus_tone(fmt: int, n: int, seed: int, cycles_per_sample: float = 0.1234) -> np.ndarray:
    """interleaved raw samples: Gaussian noise plus one complex tone whose power is 40 dB above the noise's total power"""
    rng = np.random.default_rng(seed)
    amp = {0: 120.0, 1: 28000.0, 2: 0.5}[fmt]
    sigma = amp / np.sqrt(2e4)                                     # amp^2 = 1e4 * 2 sigma^2
    z = amp * np.exp(2j * np.pi * cycles_per_sample * np.arange(n)) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack([z.real, z.imag], axis=-1).reshape(-1)
    if fmt == 0:
        return np.clip(np.rint(127 + iq), 0, 255).astype(np.uint8)
    if fmt == 1:
        return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
    return iq.astype(np.float32)


def rel_error(got: np.ndarray, want: np.ndarray) -> float:
    """largest |got - want| / max(want, 1e-8 * max(want)): the measure the spectrum's bound is stated in"""
    return float(np.max(np.abs(got - want) / np.maximum(want, 1e-8 * np.max(want))))


# ---- scenes (fixed seeds): the transmitted scene is the reference for detection; a true carrier lies at offset_hz - cfo_hz ----------
def scene(name: str, device=None):
    """-> (raw interleaved numpy samples or torch tensor on `device`, rate, fmt, true centres in Hz, WidebandCapture or None)"""
    import torch
    from nrsc5_amd import channel, synth_wideband as sw
    dev = device or torch.device("cpu")
    if name == "A":
        offs, levels = [-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]
        st = [sw.Station(offset_hz=o, seed=500 + k, level=a) for k, (o, a) in enumerate(zip(offs, levels))]
        cap = sw.capture(st, 2400000, "cu8", n_frames=1, noise_rms=0.02, seed=3, device=dev)
    elif name == "B":
        offs = [-4.6e6, -3.0e6, -1.8e6, -1.6e6, 0.4e6, 1.2e6, 2.8e6, 4.4e6]
        levels = [1.0, 0.7, 1.0, 0.1, 0.5, 0.8, 1.0, 0.6]
        st = [sw.Station(offset_hz=o, seed=300 + k, cfo_hz=1000.0 * (k - 3), level=a, chan=channel.Impairments(host_db=20.0) if k == 5 else None)
              for k, (o, a) in enumerate(zip(offs, levels))]
        cap = sw.capture(st, 10000000, "cs16", n_frames=1, noise_rms=0.05, rms_total=6000.0, seed=8, device=dev)
    elif name == "D":
        offs, levels = [-3e6, -1e6, 1e6, 3e6], [1.0, 0.5, 0.25, 0.125]
        st = [sw.Station(offset_hz=o, seed=900 + k, level=a) for k, (o, a) in enumerate(zip(offs, levels))]
        cap = sw.capture(st, 10000000, "cs16", n_frames=1, noise_rms=0.4, seed=4, device=dev)
    elif name == "C":
        return scene_decoys(device)
    else:
        raise ValueError(name)
    return cap.raw, int(cap.rate), cap.fmt, [s.offset_hz - s.cfo_hz for s in cap.stations], cap


def scene_decoys(device=None):
    """C: no HD station at all -- noise, two analog-only FM carriers 400 kHz apart and a CW tone"""
    from nrsc5_amd import channel
    rate, n = 10000000, 2000000
    rng = np.random.default_rng(77)
    t = np.arange(n)
    x = 0.05 / np.sqrt(2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, tones in ((-2.0e6, (1000.0, 6300.0, 13700.0)), (-1.6e6, (700.0, 5100.0, 12100.0))):
        imp = channel.Impairments(host_dev_hz=75e3, host_tones_hz=tones)
        x += channel.host_carrier(n, float(rate), imp) * np.exp(2j * np.pi * f * t / rate)
    x += 0.5 * np.exp(2j * np.pi * 3.0e6 * t / rate)
    x *= 6000.0 / np.sqrt(np.mean(np.abs(x) ** 2))
    raw = np.clip(np.rint(np.stack([x.real, x.imag], axis=-1).reshape(-1)), -32768, 32767).astype(np.int16)
    if device is not None:
        import torch
        raw = torch.from_numpy(raw).to(device)
    return raw, rate, "cs16", [], None
