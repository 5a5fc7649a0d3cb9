"""Cost of delivering the audio programs in a WidebandReceiver session: K hybrid-FM stations (nrsc5_amd/synth_wideband.py, 200 kHz grid,
--frames L1 frames each) in a 20 MS/s cs16 band, pushed in --chunk samples.  Per K one JSON line with the wall time of the same
session three ways, --reps times each, alternating:
    off      WidebandReceiver(programs=False)
    native   programs=True: one eng.feed_hdc_batch call (nrsc5hip_hdc_feed) per push over all stations
    python   programs=True with the per-stream Python loop eng.feed_hdc in place of the native call
and both ratios, on / off (median native / median off) and python-loop / native -- of the whole session and of the feed alone (the
wall time spent inside the receiver's feed step, which the session's other work does not dilute).  For the native case the line
also says how much of the feed step is the library call (index launch, copy, consumer, packet callbacks) and how much the receiver's
own distribution of the packets.  The three sessions must deliver the same packets.
Noise would not do here (tools/gpu_trim_bench.py): without stations there are no frames to index and no packets.
`python tools/gpu_programs_bench.py [--k 8,32] [--frames 3] [--out profiles/wideband_programs.jsonl]`"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def python_loop_feed(rx, eng):
    """the receiver's feed step with eng.feed_hdc per station instead of the one native call"""
    def feed(fresh):
        rx.hdc.events.clear()
        for s in range(rx.k):
            if len(fresh[s]):
                eng.feed_hdc(rx.engine, rx.hdc, s, fresh[s])
        for s, program, count, flags, data in rx.hdc.events:
            rx.packets[s].append((program, flags, data))
        rx.hdc.events.clear()
    return feed


def session(wideband, eng, torch, cap, offs, chunk, mode):
    """-> (wall s of all pushes, wall s inside the feed step, wall s inside the library call, packets, digest of the packets)"""
    n = cap.raw.numel() // 2
    q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offs, q15_capacity=q15, programs=mode != "off")
    spent = {"feed": 0.0, "call": 0.0}
    if mode != "off":
        inner = python_loop_feed(rx, eng) if mode == "python" else rx._feed_programs

        def timed(fresh):
            t0 = time.perf_counter()
            inner(fresh)
            spent["feed"] += time.perf_counter() - t0
        rx._feed_programs = timed
        if mode == "native":
            call0 = eng.feed_hdc_batch

            def timed_call(*args, **kw):
                t0 = time.perf_counter()
                out = call0(*args, **kw)
                spent["call"] += time.perf_counter() - t0
                return out
            eng.feed_hdc_batch = timed_call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        for p in range(0, n, chunk):
            rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        if mode == "native":
            eng.feed_hdc_batch = call0
    h = hashlib.sha256()
    for s in range(rx.k):
        for program, flags, data in rx.packets[s]:
            h.update(b"%d %d %d %d " % (s, program, flags, len(data)))
            h.update(data)
    npk = sum(len(p) for p in rx.packets)
    nrec = sum(len(rx.station_records(s)) for s in range(rx.k))
    rx.close()
    return wall, spent["feed"], spent["call"], npk, h.hexdigest()[:16], nrec


def main():
    import numpy as np
    import torch
    from nrsc5_amd import engine as eng, synth_wideband as sw, wideband
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--frames", type=int, default=3, help="L1 frames per station (1.486 s each)")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    med = lambda v: sorted(v)[len(v) // 2]
    for k in [int(v) for v in a.k.split(",")]:
        edge = a.rate / 2 - 198.5e3
        offs = [float(v) for v in np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)]
        rng = np.random.default_rng(k)
        st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320))) for i, o in enumerate(offs)]
        cap = sw.capture(st, a.rate, "cs16", n_frames=a.frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=dev)
        torch.cuda.synchronize()
        session(wideband, eng, torch, cap, offs, a.chunk, "native")          # warm-up: first launches, staging buffers
        modes = ("off", "native", "python")
        wall = {m: [] for m in modes}
        feed = {m: [] for m in modes}
        call, packets, digests, nrec = [], set(), set(), 0
        for rep in range(a.reps):
            for m in modes:
                w, f, c, npk, dg, nrec = session(wideband, eng, torch, cap, offs, a.chunk, m)
                wall[m].append(w)
                feed[m].append(f)
                if m == "native":
                    call.append(c)
                if m != "off":
                    packets.add(npk)
                    digests.add(dg)
        assert len(digests) == 1 and len(packets) == 1, (digests, packets)     # native and Python loop delivered the same packets, every time
        n = cap.raw.numel() // 2
        line = {"metric": "wideband_programs", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": -(-n // a.chunk),
                "session_signal_s": round(n / a.rate, 2), "sessions": a.reps, "records": nrec, "packets": packets.pop(),
                "session_wall_s": {m: [round(v, 3) for v in wall[m]] for m in modes},
                "feed_wall_s": {m: [round(v, 4) for v in feed[m]] for m in modes if m != "off"},
                "native_library_call_wall_s": [round(v, 4) for v in call],
                "on_over_off": round(med(wall["native"]) / med(wall["off"]), 4),
                "python_loop_over_native_session": round(med(wall["python"]) / med(wall["native"]), 4),
                "python_loop_over_native_feed": round(med(feed["python"]) / med(feed["native"]), 2),
                "feed_share_of_native_session": round(med(feed["native"]) / med(wall["native"]), 4),
                "library_call_share_of_feed": round(med(call) / med(feed["native"]), 4),
                "times_real_time_native": round(n / a.rate / med(wall["native"]), 2),
                "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes}, "source_sha": sha}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
