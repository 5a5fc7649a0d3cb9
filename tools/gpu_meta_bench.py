"""Cost of the now-playing metadata in a WidebandReceiver session, next to the cost of the audio programs: K hybrid-FM stations
(nrsc5_amd/synth_wideband.py, 200 kHz grid, --frames L1 frames each, every station with a PSD stream of ID3 packets) in a 20 MS/s cs16
band, pushed in --chunk samples.  Per K one JSON line with the wall time of the same session three ways, --reps times each, alternating:
    off        WidebandReceiver()
    programs   programs=True: nrsc5hip_hdc_feed per push -- index structs and PDU bytes of every frame copied to the host
    metadata   metadata=True: nrsc5hip_psd_feed per push -- the frames stay on the device, finished AAS packets come back
with the spread of the repeats, the share of each session spent in its feed step, and the bytes each feed moved device -> host
(metadata: nrsc5hip_psd_stats [9]; programs: the index structs and the PDU bytes at the call's stride, computed from the records).
`python tools/gpu_meta_bench.py [--k 8,32] [--frames 3] [--out profiles/wideband_metadata.jsonl]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def psd_stream(k: int, frames: int) -> bytes:
    from nrsc5_amd import synth_l2 as pa
    out, j = b"", 0
    while len(out) < 160 * frames:
        out += pa.hdlc(pa.aas_payload(0x5100, j, pa.id3_tag("Station %d song %d" % (k, j), "Artist %d" % k)))
        j += 1
    return out


def session(wideband, eng, torch, cap, offs, chunk, mode):
    """-> (wall s of all pushes, wall s inside the feed step, bytes device -> host of the feeds, packets delivered)"""
    n = cap.raw.numel() // 2
    q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offs, q15_capacity=q15, programs=mode == "programs", metadata=mode == "metadata")
    spent = {"feed": 0.0, "d2h": 0}
    name = {"programs": "_feed_programs", "metadata": "_feed_metadata"}.get(mode)
    if name:
        inner = getattr(rx, name)

        def timed(fresh, *rest):
            t0 = time.perf_counter()
            inner(fresh, *rest)
            spent["feed"] += time.perf_counter() - t0
            if mode == "programs":                               # what nrsc5hip_l2_index copies back: every index struct and the PDU bytes at the stride
                jobs = [j for s in range(rx.k) for j in eng.l2_jobs_from_records(s, fresh[s])]
                if jobs:
                    stride = (max(j[4] for j in jobs) // 8 + 15) & ~15
                    spent["d2h"] += len(jobs) * (eng.ctypes.sizeof(eng.L2Frame) + stride)
        setattr(rx, name, timed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(0, n, chunk):
        rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if mode == "metadata":
        spent["d2h"] = rx.psd.stats(0)["d2h_bytes"]
        npk = sum(rx.psd.stats(s)["delivered"] for s in range(rx.k))
    else:
        npk = sum(len(p) for p in rx.packets)
    rx.close()
    return wall, spent["feed"], spent["d2h"], npk


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
        st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320)), psd=psd_stream(i, a.frames))
              for i, o in enumerate(offs)]
        cap = sw.capture(st, a.rate, "cs16", n_frames=a.frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=dev)
        torch.cuda.synchronize()
        modes = ("off", "programs", "metadata")
        for m in modes[1:]:
            session(wideband, eng, torch, cap, offs, a.chunk, m)             # warm-up: first launches, staging buffers
        wall = {m: [] for m in modes}
        feed = {m: [] for m in modes}
        d2h, packets = {}, {}
        for rep in range(a.reps):
            for m in modes:
                w, f, b, npk = session(wideband, eng, torch, cap, offs, a.chunk, m)
                wall[m].append(w)
                feed[m].append(f)
                d2h[m], packets[m] = b, npk
        n = cap.raw.numel() // 2
        spread = {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes}
        added = {m: med(wall[m]) - med(wall["off"]) for m in modes[1:]}
        line = {"metric": "wideband_metadata", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": -(-n // a.chunk),
                "session_signal_s": round(n / a.rate, 2), "sessions": a.reps,
                "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes}, "spread_of_repeats": spread,
                "feed_wall_s": {m: [round(v, 4) for v in feed[m]] for m in modes[1:]},
                "feed_share_of_session": {m: round(med(feed[m]) / med(wall[m]), 4) for m in modes[1:]},
                "added_to_off_s": {m: round(v, 4) for m, v in added.items()},
                "d2h_bytes": {m: d2h[m] for m in modes[1:]}, "packets": {m: packets[m] for m in modes[1:]},
                "metadata_adds_less_than_programs_beyond_the_spread": bool(added["programs"] - added["metadata"] > (max(spread.values()) - 1.0) * med(wall["off"])),
                "source_sha": sha}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
