"""Wideband multi-station capture generator -- TEST / BENCH SIGNAL SOURCE ONLY, like synth_torch.py.

K hybrid-FM MP1 stations (or, with digital=False, analog-only FM stations: the host alone), each: clean baseband from synth_torch.modulate at 1 488 375 S/s with its own payload seed, an optional
channel (channel.Impairments, e.g. an analog host), a carrier offset, a timing offset, the receiver-side conjugation synth / synth_torch
apply, an optional analog FM stereo host (synth_fm), an FFT (zero-padding) resampler to Fs_in, a shift to +f_k and a level; the stations are summed, white noise is added and the
result is quantised to cu8, cs16 or cf32.  float64 (complex128) throughout, fixed seeds."""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

from . import synth, synth_torch

BAND_HZ = 198.5e3


@dataclass
class Station:
    offset_hz: float                     # f_k: centre relative to the capture centre
    seed: int                            # payload seed (synth_torch.payload_stream)
    cfo_hz: float = 0.0                  # carrier offset of the transmitter, |cfo| <= 3 kHz
    level: float = 1.0                   # rms amplitude relative to the other stations
    timing: int = 0                      # leading samples at 1 488 375 S/s before the transmission starts
    chan: object = None                  # channel.Impairments or None
    psd: bytes | None = None             # program 0's PSD byte stream (synth_torch.payload_stream), None: flag bytes only
    pids: object = None                  # the PIDS frames to transmit, cycled ([n, 80] bits, synth.sis_frame), None: reserved-id frames only
    host: dict | None = None             # analog FM host in the middle of the station: synth_fm.fm_carrier's programme (left, right, pilot, preemph_us, rds, same, rays, ...)
    host_db: float = 20.0                # ... its carrier power over the total digital power, dB
    digital: bool = True                 # False: an analog-only station, the host alone at `level` (host_db has nothing to refer to)


@dataclass
class WidebandCapture:
    raw: torch.Tensor                    # interleaved samples in the capture's format, on the device
    rate: Fraction
    fmt: str
    stations: list
    p1: list = field(default_factory=list)      # per station: transmitted P1 frames [F, 146176] u8
    pids: list = field(default_factory=list)    # per station: transmitted PIDS frames [16 F, 80] u8
    snr_db: list = field(default_factory=list)  # per station: rms over the noise in +-198.5 kHz


def _smooth(n: int) -> int:
    """smallest 2^a 3^b 5^c >= n"""
    best = 1 << max(0, int(n - 1).bit_length())
    p5 = 1
    while p5 < 2 * n:
        p35 = p5
        while p35 < 2 * n:
            v = p35
            while v < n:
                v *= 2
            best = min(best, v)
            p35 *= 3
        p5 *= 5
    return best


def fft_resample(x: torch.Tensor, ratio: Fraction) -> torch.Tensor:
    """band-limited resampling of a complex128 signal by the exact ratio num / den (output rate / input rate), zero-padding (or
    truncating) its spectrum; the input is zero-extended to a length whose output length is an integer"""
    num, den = ratio.numerator, ratio.denominator
    k = _smooth(-(-x.shape[0] // den))
    n_in, n_out = k * den, k * num
    xp = torch.zeros(n_in, dtype=torch.complex128, device=x.device)
    xp[:x.shape[0]] = x
    X = torch.fft.fft(xp)
    Y = torch.zeros(n_out, dtype=torch.complex128, device=x.device)
    h = min(n_in, n_out) // 2
    Y[:h] = X[:h]
    Y[-h:] = X[-h:]
    return torch.fft.ifft(Y) * (n_out / n_in)


def capture(stations, rate, fmt: str = "cs16", n_frames: int = 3, noise_rms: float = 0.002, rms_total: float | None = None,
            seed: int = 0, device=None) -> WidebandCapture:
    """rms_total: rms of the capture before quantisation (default: 3000 LSB cs16, 0.09 cf32, 25 counts cu8)"""
    dev = device or torch.device("cuda", 0)
    rate = Fraction(rate)
    ratio = rate / Fraction(synth.FS_CU8).limit_denominator(4)
    out = None
    cap = WidebandCapture(None, rate, fmt, list(stations))
    fs_in = float(rate)
    for st in stations:
        if not st.digital:                                   # the host alone, as long as a digital station's transmission; no frames
            from . import synth_fm
            n0 = n_frames * 512 * 4320                       # 512 symbols of 4320 samples at 1 488 375 S/s per L1 frame
            car = synth_fm.fm_carrier(n0, fs=synth.FS_CU8, **(st.host or {})) * np.exp(-2j * np.pi * st.cfo_hz / synth.FS_CU8 * np.arange(n0))
            sig = torch.from_numpy(car).to(dev)
            p1, pids = np.zeros((0, 146176), dtype=np.uint8), np.zeros((0, 80), dtype=np.uint8)
        else:
            p1, pids, m = synth_torch.payload_stream(n_frames, seed=st.seed, psd_stream=st.psd, pids=st.pids)
            sig = synth_torch.modulate(m, dev)
            if st.chan is not None:
                from . import channel
                sig = channel.apply_torch(sig, synth.FS_CU8, st.chan)
            sig = sig.to(torch.complex128)
            n0 = sig.shape[0]
            t = torch.arange(n0, device=dev, dtype=torch.float64)
            sig = sig * torch.exp(1j * (2 * np.pi * st.cfo_hz / synth.FS_CU8) * t)
            sig = sig.conj()
        if st.digital and st.host is not None:                              # as transmitted (the conjugation above is the digital receiver's), with the station's carrier offset
            from . import synth_fm
            amp = float(torch.sqrt(torch.mean(torch.abs(sig) ** 2))) * 10 ** (st.host_db / 20)
            car = synth_fm.fm_carrier(n0, fs=synth.FS_CU8, **st.host) * np.exp(-2j * np.pi * st.cfo_hz / synth.FS_CU8 * np.arange(n0))
            sig = sig + amp * torch.from_numpy(car).to(dev)
        sig = torch.cat([torch.zeros(st.timing, dtype=torch.complex128, device=dev), sig,
                         torch.zeros(8640, dtype=torch.complex128, device=dev)])
        y = fft_resample(sig, ratio)
        y = y[:int(sig.shape[0] * ratio)]
        tt = torch.arange(y.shape[0], device=dev, dtype=torch.float64)
        y = y * st.level / torch.sqrt(torch.mean(torch.abs(y) ** 2)) * torch.exp(1j * torch.remainder(2 * np.pi * st.offset_hz / fs_in * tt, 2 * np.pi))
        if out is None:
            out = y
        else:
            if y.shape[0] > out.shape[0]:
                y, out = out, y
            out[:y.shape[0]] += y
        cap.p1.append(p1)
        cap.pids.append(pids)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    noise = torch.complex(torch.randn(out.shape[0], generator=g, device=dev, dtype=torch.float64),
                          torch.randn(out.shape[0], generator=g, device=dev, dtype=torch.float64)) * (noise_rms / np.sqrt(2))
    out = out + noise
    in_band = noise_rms ** 2 * 2 * BAND_HZ / fs_in
    cap.snr_db = [10 * np.log10(st.level ** 2 / in_band) for st in stations]
    default = {"cs16": 3000.0, "cf32": 0.09, "cu8": 25.0}[fmt]
    scale = (rms_total or default) / float(torch.sqrt(torch.mean(torch.abs(out) ** 2)))
    out = out * scale
    iq = torch.stack([out.real, out.imag], dim=1).reshape(-1)
    if fmt == "cs16":
        raw = torch.clamp(torch.round(iq), -32768, 32767).to(torch.int16)
    elif fmt == "cu8":
        raw = torch.clamp(torch.round(127 + iq), 0, 255).to(torch.uint8)
    else:
        raw = iq.to(torch.float32)
    cap.raw = raw
    return cap
