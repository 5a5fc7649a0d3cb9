"""Cost of nrsc5hip_batch_trim in a WidebandReceiver session: K stations on the 200 kHz grid of a 20 MS/s cs16 band, default FIFO
capacity (1 << 24 samples per station) and push (1 << 22 samples), the same push repeated until the session is --fifos times the
FIFO.  Per K one JSON line: device time of one trim (HIP events around the call on the engine's stream) and its wall time, the bytes
it moved, the pushes between two trims, and the trims' share of the session's wall time next to chan.feed + batch_process of the
same run; then the same session through a receiver whose FIFO holds everything and never trims -- the reference for "no cost".
Both sessions are repeated --reps times, alternating, and every wall time is reported: the spread between repeats of ONE kind is
what the difference between the two kinds has to be read against.
The band is noise (as in tools/gpu_wideband_bench.py): what a trim moves does not depend on what the samples say.
`python tools/gpu_trim_bench.py [--k 8,32,64] [--fifos 2.5] [--out profiles/wideband_trim.jsonl]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def session(rx, x, pushes, torch):
    """-> wall seconds of the pushes, and of the trims inside them: (wall ms, device ms, bytes moved) per trim"""
    from nrsc5_amd import engine as eng
    stream = torch.cuda.ExternalStream(rx.engine.hip_stream)
    trims = []
    trim0 = rx.engine.batch_trim

    def timed_trim(n, stream_ids=None):
        held = rx.held
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        kept = trim0(n, stream_ids=stream_ids)
        wall = time.perf_counter() - t0
        b.record(stream)
        b.synchronize()
        trims.append((1e3 * wall, a.elapsed_time(b), int(4 * kept.sum()), held, int(kept.max())))
        return kept

    rx.engine.batch_trim = timed_trim
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(pushes):
        rx.push(x)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rx.engine.batch_trim = trim0
    assert eng.TRIM_RETAIN_MAX >= rx.max_retained
    return wall, trims


def main():
    import numpy as np
    import torch
    from nrsc5_amd import engine as eng, wideband
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32,64")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--fifos", type=float, default=2.5, help="length of the session in FIFO capacities")
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.clamp(torch.randn(2 * a.chunk, generator=g, device=dev) * 3000, -32768, 32767).to(torch.int16)
    torch.cuda.synchronize()
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for k in [int(v) for v in a.k.split(",")]:
        edge = a.rate / 2 - 198.5e3
        offs = np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)
        per_push = a.chunk * 744187.5 / a.rate
        pushes = int(a.fifos * a.capacity / per_push) + 1
        walls = {"trimmed": [], "holds_everything": []}
        trims, n_push = [], 0
        for rep in range(a.reps):
            for name, cap in (("trimmed", a.capacity), ("holds_everything", int(pushes * per_push) + 4 * 71280)):
                rx = wideband.WidebandReceiver(a.rate, "cs16", offs, q15_capacity=cap)
                rx.push(x)                                               # warm-up: first launches, staging buffers
                wall, tr = session(rx, x, pushes - 1, torch)
                walls[name].append(wall)
                if name == "trimmed":
                    trims += tr
                    n_push = rx.pushes
                else:
                    assert not tr
                rx.close()
        assert trims
        w, wr = walls["trimmed"], walls["holds_everything"]
        med = lambda v: sorted(v)[len(v) // 2]
        line = {"metric": "wideband_trim", "rate": a.rate, "channels": k, "q15_capacity": a.capacity, "chunk": a.chunk, "pushes": n_push,
                "session_signal_s": round(n_push * a.chunk / a.rate, 1), "sessions": a.reps, "trims_per_session": len(trims) // a.reps,
                "pushes_between_trims": round(a.capacity / per_push, 1),
                "trim_device_ms": [round(t[1], 3) for t in trims], "trim_wall_ms": [round(t[0], 3) for t in trims],
                "trim_bytes_moved": [t[2] for t in trims], "retained_max_samples": max(t[4] for t in trims),
                "session_wall_s": [round(v, 3) for v in w], "trim_share_of_wall": round(sum(t[0] for t in trims) / 1e3 / sum(w), 6),
                "session_wall_s_without_trim": [round(v, 3) for v in wr], "median_wall_ratio_to_no_trim": round(med(w) / med(wr), 4),
                "spread_of_repeats": [round(max(w) / min(w), 4), round(max(wr) / min(wr), 4)], "source_sha": sha}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
