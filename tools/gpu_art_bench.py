"""Cost of the data services (SIG, LOT files: album art, station logos) in a WidebandReceiver session, next to the metadata alone, and what a repeating
carousel does to the host.  Two legs, one JSON line each per K:
    session    K hybrid-FM stations (nrsc5_amd/synth_wideband.py, 200 kHz grid, --frames L1 frames each) in a 20 MS/s cs16 band, pushed in --chunk
               samples; every station's PSD stream holds an ID3 tag, its SIG and a small file, repeated (the generators carry 160 PSD bytes per L1 frame,
               so a file here is --file-bytes long).  The same session two ways, --reps times each, alternating:
                   metadata        metadata=True: nrsc5hip_psd_feed per push -- every AAS packet comes back, those of other ports are kept in aas[s]
                   data_services   data_services=True: nrsc5hip_aas_feed per push -- k_aas chained behind k_psd, only events come back
               wall time per push, bytes device -> host per mode, host bytes held at the end (aas[s] / files[s]).
    carousel   a carousel of realistic size -- the SIG, an ID3 tag and files of --files bytes per station, --rounds times over -- as P1 frames with 2360
               PSD bytes each through the stage hooks of the same two paths (nrsc5hip_stage_psd_streams; nrsc5hip_stage_aas_frames), K streams per call,
               a round per call: wall time per call, bytes device -> host per round, host bytes held at the end.
`python tools/gpu_art_bench.py [--k 8,32] [--frames 4] [--out profiles/wideband_art.jsonl]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOT_PORT, MIME_ART = 0x1000, 0xBE4B7536


def station_sig(k: int) -> bytes:
    from nrsc5_amd import synth_l2 as sl
    return sl.sig_service(1, audio=True) + sl.sig_name(b"MPS") + sl.sig_audio(0, 0, 14) + sl.sig_data(1, LOT_PORT + k, 3, MIME_ART)


def file_body(k: int, j: int, n: int) -> bytes:
    import numpy as np
    return np.random.default_rng(1000 * k + j).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def carousel_packets(k: int, sizes, seq0: int = 0) -> list:
    from nrsc5_amd import synth_l2 as sl
    out = [(0x5100, seq0 + 1, sl.id3_tag("Station %d" % k, "Artist %d" % k)), (0x20, seq0, station_sig(k))]
    for j, n in enumerate(sizes):
        out += sl.lot_file_packets(LOT_PORT + k, 100 + j, file_body(k, j, n), b"art%d_%d.jpg" % (k, j), MIME_ART, seq0 + 2 + 100 * j)
    return out


def psd_stream(k: int, frames: int, file_bytes: int) -> bytes:
    from nrsc5_amd import synth_l2 as sl
    out, j = b"", 0
    while len(out) < 160 * frames:
        out += b"".join(sl.hdlc(sl.aas_payload(*p)) for p in carousel_packets(k, (file_bytes,), 10 * j))
        j += 1
    return out


def held_bytes(rx) -> int:
    return sum(len(p[3]) for per in rx.aas for p in per) + sum(len(f["data"]) + len(f["name"]) for per in rx.files for f in per.values())


def session(wideband, torch, cap, offs, chunk, mode):
    """-> (wall s of all pushes, wall s inside the feed step, bytes device -> host of the feeds, host bytes held at the end, files delivered)"""
    n = cap.raw.numel() // 2
    q15 = int(n / float(cap.rate) * 744187.5) + 4 * 71280
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offs, q15_capacity=q15, metadata=True, data_services=mode == "data_services")
    spent = {"feed": 0.0}
    name = "_feed_data_services" if mode == "data_services" else "_feed_metadata"
    inner = getattr(rx, name)

    def timed(fresh, *rest):
        t0 = time.perf_counter()
        inner(fresh, *rest)
        spent["feed"] += time.perf_counter() - t0
    setattr(rx, name, timed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(0, n, chunk):
        rx.push(cap.raw[2 * p:2 * min(n, p + chunk)])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    d2h = rx.psd.stats(0)["d2h_bytes"] + (rx.data.stats(0)["d2h_bytes"] if rx.data is not None else 0)
    out = wall, spent["feed"], d2h, held_bytes(rx), sum(len(f) for f in rx.files)
    rx.close()
    return out


def carousel(eng, k, sizes, rounds, mode, lib_path=None):
    """-> (wall s per call, bytes device -> host per round, host bytes held at the end, files delivered, frames per round)"""
    from nrsc5_amd import synth_l2 as sl
    E = eng.Engine(max_streams=1, q15_capacity=200000, record_capacity=64, p1_slots=2, lib_path=lib_path)
    P = eng.PsdConsumer(E, k)
    A = eng.AasConsumer(E, k, lot_files=16) if mode == "data_services" else None
    frames = [sl.aas_frames(carousel_packets(s, sizes)) for s in range(k)]
    targets, lcs = list(range(k)), [0] * k
    walls, moved, kept, files = [], [], 0, 0
    d2h = lambda: P.stats(0)["d2h_bytes"] + (A.stats(0)["d2h_bytes"] if A is not None else 0)
    for r in range(rounds + 1):                                  # the first call is the warm-up: its time is dropped, its files are the ones delivered
        if r == 1 and A is not None:
            for s in range(k):
                A.reset(s)
        before = d2h()
        t0 = time.perf_counter()
        if A is not None:
            ev = A.stage_frames(P, targets, frames, lcs)
            new = sum(len(f["data"]) + len(f["name"]) for _, kind, f in ev if kind == "lot")
            nfiles = sum(1 for _, kind, _ in ev if kind == "lot")
            A.events.clear(); A.raw.clear()
        else:
            pk = P.stage_streams(targets, frames, lcs)
            new = sum(len(p[4]) for p in pk if not (p[2] == 0x5100 or 0x5201 <= p[2] <= 0x5207))      # what the receiver keeps in aas[s]
            nfiles = 0
            P.packets.clear()
        if r:
            walls.append(time.perf_counter() - t0)
            moved.append(d2h() - before)
            kept += new
            files += nfiles
    for c in (A, P):
        if c is not None:
            c.close()
    E.close()
    return walls, moved, kept, files, sum(len(f) for f in frames)


def main():
    import numpy as np
    import torch
    from nrsc5_amd import engine as eng, synth_wideband as sw, wideband
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--frames", type=int, default=4, help="L1 frames per station (1.486 s each); a receiver may lose the first, and a round of the stream is about 300 bytes")
    ap.add_argument("--file-bytes", type=int, default=150, help="session leg: bytes of the file every station repeats")
    ap.add_argument("--files", default="2000,8000,20000", help="carousel leg: bytes of the files of a station's carousel")
    ap.add_argument("--rounds", type=int, default=3, help="carousel leg: times the carousel is sent")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--legs", default="session,carousel")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    med = lambda v: sorted(v)[len(v) // 2]
    sizes = [int(v) for v in a.files.split(",")]
    modes = ("metadata", "data_services")

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    for k in [int(v) for v in a.k.split(",")]:
        if "carousel" in a.legs:
            res = {m: carousel(eng, k, sizes, a.rounds, m) for m in modes}
            emit({"metric": "wideband_art_carousel", "streams": k, "files_bytes": sizes, "rounds": a.rounds,
                  "frames_per_round": res["metadata"][4],
                  "call_wall_s": {m: [round(v, 5) for v in res[m][0]] for m in modes},
                  "d2h_bytes_per_round": {m: res[m][1] for m in modes}, "host_bytes_held": {m: res[m][2] for m in modes},
                  "files_delivered": res["data_services"][3], "source_sha": sha})
        if "session" not in a.legs:
            continue
        edge = a.rate / 2 - 198.5e3
        offs = [float(v) for v in np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)]
        rng = np.random.default_rng(k)
        st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320)),
                         psd=psd_stream(i, a.frames, a.file_bytes)) for i, o in enumerate(offs)]
        cap = sw.capture(st, a.rate, "cs16", n_frames=a.frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=dev)
        torch.cuda.synchronize()
        for m in modes:
            session(wideband, torch, cap, offs, a.chunk, m)                 # warm-up: first launches, staging buffers
        wall, feed = {m: [] for m in modes}, {m: [] for m in modes}
        d2h, held, files = {}, {}, {}
        for rep in range(a.reps):
            for m in modes:
                w, f, b, h, nf = session(wideband, torch, cap, offs, a.chunk, m)
                wall[m].append(w)
                feed[m].append(f)
                d2h[m], held[m], files[m] = b, h, nf
        n = cap.raw.numel() // 2
        pushes = -(-n // a.chunk)
        emit({"metric": "wideband_art_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": pushes, "session_signal_s": round(n / a.rate, 2),
              "sessions": a.reps, "file_bytes": a.file_bytes,
              "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes},
              "push_wall_ms": {m: round(1e3 * med(wall[m]) / pushes, 3) for m in modes},
              "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes},
              "feed_wall_s": {m: [round(v, 4) for v in feed[m]] for m in modes},
              "added_to_metadata_s": round(med(wall["data_services"]) - med(wall["metadata"]), 4),
              "d2h_bytes": d2h, "host_bytes_held": held, "files_delivered": files["data_services"], "source_sha": sha})
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
