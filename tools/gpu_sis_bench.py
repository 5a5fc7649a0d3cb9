"""Cost of the station information (SIS) in a WidebandReceiver session, next to the audio programs and the now-playing metadata: K hybrid-FM
stations (nrsc5_amd/synth_wideband.py, 200 kHz grid, --frames L1 frames each, every station with a PSD stream of ID3 packets and a SIS schedule of
its own) in a 20 MS/s cs16 band, pushed in --chunk samples.  Per K one JSON line with the wall time of the same session five ways, --reps times
each, alternating:
    off        WidebandReceiver()
    sis        sis=True: nrsc5hip_sis_feed per push -- 16 bytes per record up, one k_sis launch, the events back
    metadata   metadata=True: nrsc5hip_psd_feed per push
    programs   programs=True: nrsc5hip_hdc_feed per push
    all        the three together
with the spread of the repeats, the share of each session spent in its SIS feed, the bytes the SIS and PSD feeds moved device -> host
(nrsc5hip_sis_stats [30], nrsc5hip_psd_stats [9]) and the events delivered.  The `off` leg is the session of tools/gpu_meta_bench.py's `off` leg.
`python tools/gpu_sis_bench.py [--k 8,32] [--frames 3] [--out profiles/wideband_sis.jsonl]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"off": {}, "sis": {"sis": True}, "metadata": {"metadata": True}, "programs": {"programs": True},
         "all": {"sis": True, "metadata": True, "programs": True}}


def sis_frames(k: int):
    """a station's PIDS frames: id, names, slogan, a message, location, service descriptors, parameters; every station its own call sign"""
    from nrsc5_amd import synth as S
    name = "K%c%c%c" % (65 + k % 26, 65 + k // 26 % 26, 65 + (7 * k) % 26)
    groups = [[S.sis_station_id("US", 10000 + k), S.sis_short_name(name, True)]]
    groups += [[p] for p in S.sis_long_name(b"%s wideband" % name.encode(), seq=k % 8)]
    groups += [[p] for p in S.sis_message(b"Station %d is on the air" % k, seq=k % 4)]
    groups += [[p] for p in S.sis_universal_name(name.encode() + b"-HD")]
    groups += [list(S.sis_location(int(40.0 * 8192) + k, int(-75.0 * 8192) - k, 16 * k))]
    groups += [[S.sis_audio_service(p, 0, 1 + p + k % 5, 0), S.sis_data_service(0, 64 + p, 0x100 + p + k)] for p in range(3)]
    groups += [[S.sis_parameter(i, 0x0101 * (i + 1) + k), S.sis_parameter(i + 1, 0x0203 + i + k)] for i in range(0, 12, 2)]
    import numpy as np
    return np.stack([S.sis_frame(g) for g in groups])


def session(wideband, torch, cap, offs, chunk, mode):
    """-> (wall s of all pushes, wall s inside the SIS feed, {"sis", "psd"} bytes device -> host, SIS events, AAS packets, HDC packets)"""
    n = cap.raw.numel() // 2
    q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offs, q15_capacity=q15, **MODES[mode])
    spent = {"feed": 0.0}
    if rx.sis is not None:
        inner = rx._feed_sis

        def timed(fresh, events):
            t0 = time.perf_counter()
            inner(fresh, events)
            spent["feed"] += time.perf_counter() - t0
        rx._feed_sis = timed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(0, n, chunk):
        rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    d2h = {"sis": rx.sis.stats(0)["d2h_bytes"] if rx.sis is not None else 0, "psd": rx.psd.stats(0)["d2h_bytes"] if rx.psd is not None else 0}
    events = sum(rx.sis.stats(s)["events"] for s in range(rx.k)) if rx.sis is not None else 0
    named = sum(1 for i in rx.station_info if i is not None and i["name"] is not None)
    aas = sum(rx.psd.stats(s)["delivered"] for s in range(rx.k)) if rx.psd is not None else 0
    hdc = sum(len(p) for p in rx.packets)
    rx.close()
    return wall, spent["feed"], d2h, events, named, aas, hdc


def main():
    import numpy as np
    import torch
    from nrsc5_amd import engine as eng, synth_wideband as sw, wideband
    from tools.gpu_meta_bench import psd_stream
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
    modes = list(MODES)
    for k in [int(v) for v in a.k.split(",")]:
        edge = a.rate / 2 - 198.5e3
        offs = [float(v) for v in np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)]
        rng = np.random.default_rng(k)
        st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320)), psd=psd_stream(i, a.frames),
                         pids=sis_frames(i)) for i, o in enumerate(offs)]
        cap = sw.capture(st, a.rate, "cs16", n_frames=a.frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=dev)
        torch.cuda.synchronize()
        for m in modes[1:]:
            session(wideband, torch, cap, offs, a.chunk, m)                  # warm-up: first launches, staging buffers
        wall = {m: [] for m in modes}
        feed, d2h, counts = {m: [] for m in modes}, {}, {}
        for rep in range(a.reps):
            for m in modes:
                w, f, b, ev, named, aas, hdc = session(wideband, torch, cap, offs, a.chunk, m)
                wall[m].append(w)
                feed[m].append(f)
                d2h[m], counts[m] = b, {"sis_events": ev, "stations_named": named, "aas_packets": aas, "hdc_packets": hdc}
        n = cap.raw.numel() // 2
        spread = {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes}
        added = {m: med(wall[m]) - med(wall["off"]) for m in modes[1:]}
        line = {"metric": "wideband_sis", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": -(-n // a.chunk),
                "session_signal_s": round(n / a.rate, 2), "sessions": a.reps,
                "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes}, "spread_of_repeats": spread,
                "added_to_off_s": {m: round(v, 4) for m, v in added.items()},
                "sis_feed_wall_s": {m: [round(v, 4) for v in feed[m]] for m in ("sis", "all")},
                "sis_feed_share_of_session": {m: round(med(feed[m]) / med(wall[m]), 4) for m in ("sis", "all")},
                "d2h_bytes": {m: d2h[m] for m in modes[1:]}, "delivered": {m: counts[m] for m in modes[1:]},
                "sis_adds_more_than_the_spread_of_off": bool(added["sis"] > (spread["off"] - 1.0) * med(wall["off"])),
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
