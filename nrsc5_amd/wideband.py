"""Decode every listed HD station of one wideband SDR capture: the channelizer (nrsc5hip_chan_*) feeds one engine stream per station,
and the batch engine decodes them (p1_async, l2_feedback).

    python -m nrsc5_amd.wideband FILE --format cs16 --rate 20000000 --offsets -800e3,0,400e3

prints one line per station event (SYNC with its frequency offset, MER, BER, LOST_SYNC)."""
from __future__ import annotations

import argparse
import sys
from fractions import Fraction

import numpy as np

from . import engine as eng


class WidebandReceiver:
    """rate: S/s (int, Fraction or float); fmt: "cu8" | "cs16" | "cf32"; offsets_hz: one station centre per entry, relative to the
    capture centre.  push() takes interleaved samples as a host numpy array or a torch tensor on the device; every push decodes what
    it completes, and each station's events (records_to_log's ordered log, frames included) accumulate in `logs[k]`.
    q15_capacity: 744 187.5 S/s samples each station's engine stream holds -- the whole session's (the replay of l2_feedback
    needs the samples since a frame's first block; size it for the capture)."""

    def __init__(self, rate, fmt: str, offsets_hz, device: int = 0, gains=None, q15_capacity: int = 1 << 24, lib_path: str | None = None):
        import torch
        self.fmt = eng.IQ_FORMATS[fmt]
        self.dtype = eng.IQ_DTYPES[self.fmt]
        self.dev = torch.device("cuda", device)
        self.offsets = [float(f) for f in offsets_hz]
        self.k = len(self.offsets)
        self.chan = eng.Channelizer(Fraction(rate) if not isinstance(rate, float) else rate, self.fmt, self.offsets, gains=gains,
                                    device=device, lib_path=lib_path)
        self.engine = eng.Engine(max_streams=self.k, q15_capacity=q15_capacity, record_capacity=512, p1_slots=16, p1_async=True,
                                 l2_feedback=True, device=device, lib_path=lib_path)
        self.ids = np.arange(self.k, dtype=np.int32)
        self.logs = [[] for _ in range(self.k)]
        self.records = [[] for _ in range(self.k)]

    def push(self, chunk) -> list:
        """-> the events this push produced: [(station, kind, fields), ...] in stream order per station"""
        import torch
        if isinstance(chunk, np.ndarray):
            chunk = torch.from_numpy(np.ascontiguousarray(chunk, dtype=self.dtype)).to(self.dev)
        chunk = chunk.contiguous()
        torch.cuda.current_stream(chunk.device).synchronize()      # the channelizer works on its own stream
        n = chunk.numel() // 2
        self.chan.feed(self.engine, self.ids, chunk.data_ptr(), n)
        self.engine.batch_process(self.k, stream_ids=self.ids)
        new = []
        for s in range(self.k):
            recs = self.engine.drain(s)
            if len(recs):
                log = eng.records_to_log(self.engine, s, recs)          # frames are fetched now, while their ring slots hold them
                self.logs[s] += log
                self.records[s].append(recs)
                new += [(s, kind, v) for kind, v in log]
        return new

    def station_records(self, s: int) -> np.ndarray:
        return np.concatenate(self.records[s]) if self.records[s] else np.zeros(0, dtype=eng.RECORD_DTYPE)

    def close(self):
        self.engine.close()
        self.chan.close()


def format_event(rx: WidebandReceiver, s: int, kind: str, v: dict) -> str | None:
    head = f"station {s} ({rx.offsets[s] / 1e3:+.1f} kHz):"
    if kind == "sync":
        return f"{head} SYNC freq_offset={v['freq_offset']:.1f} Hz psmi={v['psmi']}"
    if kind == "mer":
        return f"{head} MER lower={v['lower']:.1f} dB upper={v['upper']:.1f} dB"
    if kind == "ber":
        return f"{head} BER {v['cber']:.6f}"
    if kind == "lost_sync":
        return f"{head} LOST_SYNC"
    return None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m nrsc5_amd.wideband", description=__doc__.splitlines()[0])
    ap.add_argument("file")
    ap.add_argument("--format", choices=sorted(eng.IQ_FORMATS), default="cs16")
    ap.add_argument("--rate", required=True, help="S/s, an integer or a fraction num/den")
    ap.add_argument("--offsets", required=True, help="comma-separated station centres in Hz relative to the capture centre")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=1 << 22, help="samples per push")
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):                  # "--offsets -800e3,0,400e3": a value that starts with '-' is still the value
        if argv[i] == "--offsets":
            argv[i:i + 2] = ["--offsets=" + argv[i + 1]]
            break
    a = ap.parse_args(argv)
    rate = Fraction(a.rate)
    offsets = [float(x) for x in a.offsets.split(",") if x]
    fmt = eng.IQ_FORMATS[a.format]
    dtype = eng.IQ_DTYPES[fmt]
    import os
    total = os.path.getsize(a.file) // (2 * np.dtype(dtype).itemsize)
    q15 = int(total / float(rate) * 744187.5) + 4 * 71280
    rx = WidebandReceiver(rate, a.format, offsets, device=a.device, q15_capacity=q15)
    with open(a.file, "rb") as f:
        while True:
            buf = np.fromfile(f, dtype=dtype, count=2 * a.chunk)
            if buf.size < 2:
                break
            for s, kind, v in rx.push(buf[:buf.size - buf.size % 2]):
                line = format_event(rx, s, kind, v)
                if line:
                    print(line, flush=True)
    rx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
