"""Cost of the analog FM audio (nrsc5hip_fm_*, nrsc5hip_chan_feed_fm) in a WidebandReceiver session.  Three legs, one JSON line each per K:
    session    K hybrid-FM stations (nrsc5_amd/synth_wideband.py, 200 kHz grid, --frames L1 frames each: 5.95 s at the default 4), every one
               with a stereo host 14 dB over its sidebands, in a 20 MS/s cs16 band, pushed in --chunk samples.  The same session two ways,
               --reps times each, alternating:
                   off      the receiver as it is without the feature (nrsc5hip_chan_feed)
                   analog   analog=True: nrsc5hip_chan_feed_fm per push, the PCM copied to the host
               wall time per session and per push, the medians, and what analog adds.
    stage      the same pushes through the channelizer alone (Channelizer.process_tensor) and through the demodulator alone (FmDemod.process_tensor
               on the channelizer's output): wall time per push, the medians -- do the new kernels cost more than the channelizer?
    programs   the untouched programs=True session, --reps times, in a child process per tree: this one, and with --ab-tree a checkout of
               another commit (its nrsc5_amd package with its library built), alternating A B A B.
`python tools/gpu_analog_bench.py [--k 8,32] [--frames 4] [--ab-tree DIR] [--out profiles/wideband_analog.jsonl]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NRSC5_BENCH_TREE") or ROOT)      # (the programs leg's child: the package of the tree it measures)

HOST = dict(left=[(1000.0, 0.3), (4000.0, 0.1)], right=[(2500.0, 0.25)], preemph_us=75)
HOST_DB = 14.0


def scene(k: int, rate: int, frames: int, hosts: bool):
    import numpy as np
    import torch
    from nrsc5_amd import synth_wideband as sw
    edge = rate / 2 - 198.5e3
    offs = [float(v) for v in np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)]
    rng = np.random.default_rng(k)
    extra = dict(host=HOST, host_db=HOST_DB) if hosts else {}
    st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320)), **extra) for i, o in enumerate(offs)]
    cap = sw.capture(st, rate, "cs16", n_frames=frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return cap, offs


def session(cap, offs, chunk, **kw):
    """-> (wall s of all pushes, audio frames per station, events)"""
    import torch
    from nrsc5_amd import wideband
    n = cap.raw.numel() // 2
    rx = wideband.WidebandReceiver(cap.rate, cap.fmt, offs, q15_capacity=int(n / float(cap.rate) * 744187.5) + 4 * 71280, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    events = 0
    for p in range(0, n, chunk):
        events += len(rx.push(cap.raw[2 * p:2 * min(n, p + chunk)]))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    frames = sum(len(b) for b in getattr(rx, "audio", [[]])[0])
    packets = sum(len(p) for p in rx.packets)
    rx.close()
    return wall, frames, events, packets


def stage(cap, offs, chunk):
    """-> (ms per push of the channelizer alone, of the demodulator alone)"""
    import torch
    from nrsc5_amd import engine as eng
    n = cap.raw.numel() // 2
    ch = eng.Channelizer(cap.rate, eng.IQ_CS16, offs)
    fm = eng.FmDemod(len(offs))
    t_ch, t_fm = [], []
    for p in range(0, n, chunk):
        x = cap.raw[2 * p:2 * min(n, p + chunk)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = ch.process_tensor(x)
        t1 = time.perf_counter()
        fm.process_tensor(y)
        t2 = time.perf_counter()
        if 2 * (min(n, p + chunk) - p) == 2 * chunk and p:           # whole pushes behind the first (its launches load the code objects)
            t_ch.append(1e3 * (t1 - t0))
            t_fm.append(1e3 * (t2 - t1))
    ch.close(); fm.close()
    return t_ch, t_fm


def child_programs(a):
    """one tree (the one this process imports), the programs session a.reps times behind a warm-up: prints its wall times as JSON"""
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng
    k = int(a.k.split(",")[0])
    cap, offs = scene(k, a.rate, a.frames, hosts=False)
    session(cap, offs, a.chunk, programs=True)
    walls, packets = [], 0
    for _ in range(a.reps):
        w, _, _, packets = session(cap, offs, a.chunk, programs=True)
        walls.append(round(w, 4))
    print(json.dumps({"wall_s": walls, "packets": packets, "source_sha": eng.load_library().nrsc5hip_source_sha().decode()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--frames", type=int, default=4, help="L1 frames per station (1.486 s each)")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--legs", default="session,stage,programs")
    ap.add_argument("--ab-tree", default=None, help="programs leg: a checkout of another commit, library built, to run the same session with")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--child-programs", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_programs:
        return child_programs(a)
    med = lambda v: sorted(v)[len(v) // 2]

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    if "programs" in a.legs:
        k = int(a.k.split(",")[0])
        libs = [None] + ([os.path.abspath(a.ab_tree)] if a.ab_tree else [])
        runs = {lib: [] for lib in libs}
        for rnd in range(2 if a.ab_tree else 1):                     # A B A B: a fresh child process per run
            for lib in libs:
                env = dict(os.environ)
                env.pop("NRSC5_BENCH_TREE", None)
                if lib:
                    env["NRSC5_BENCH_TREE"] = lib
                cmd = [sys.executable, os.path.abspath(__file__), "--child-programs", "--rate", str(a.rate), "--k", str(k), "--frames", str(a.frames),
                       "--chunk", str(a.chunk), "--reps", str(a.reps)]
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, timeout=1500)
                if r.returncode != 0:
                    raise SystemExit("programs child failed: " + r.stderr.decode()[-2000:])
                runs[lib].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        line = {"metric": "wideband_programs_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "frames": a.frames}
        for lib, name in zip(libs, ("this_tree", "ab_tree")):
            walls = [w for run in runs[lib] for w in run["wall_s"]]
            line[name] = {"wall_s": walls, "median_s": med(walls), "packets": runs[lib][0]["packets"], "source_sha": runs[lib][0]["source_sha"]}
        if a.ab_tree:
            line["this_tree_over_ab_tree"] = round(line["this_tree"]["median_s"] / line["ab_tree"]["median_s"], 4)
        emit(line)
    if "session" not in a.legs and "stage" not in a.legs:
        return
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for k in [int(v) for v in a.k.split(",")]:
        cap, offs = scene(k, a.rate, a.frames, hosts=True)
        n = cap.raw.numel() // 2
        pushes = -(-n // a.chunk)
        if "session" in a.legs:
            modes = {"off": {}, "analog": {"analog": True}}
            for m in modes:
                session(cap, offs, a.chunk, **modes[m])                  # warm-up: first launches, staging buffers
            wall, frames = {m: [] for m in modes}, 0
            for rep in range(a.reps):
                for m in modes:
                    w, f, _, _ = session(cap, offs, a.chunk, **modes[m])
                    wall[m].append(w)
                    frames = max(frames, f)
            emit({"metric": "wideband_analog_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": pushes, "session_signal_s": round(n / a.rate, 2),
                  "sessions": a.reps, "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes},
                  "median_s": {m: round(med(wall[m]), 4) for m in modes},
                  "push_wall_ms": {m: round(1e3 * med(wall[m]) / pushes, 3) for m in modes},
                  "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes},
                  "added_by_analog_s": round(med(wall["analog"]) - med(wall["off"]), 4),
                  "audio_frames_per_station": frames, "audio_s_per_station": round(frames / 44100, 3), "source_sha": sha})
        if "stage" in a.legs:
            t_ch, t_fm = stage(cap, offs, a.chunk)
            emit({"metric": "wideband_analog_stage", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes_timed": len(t_ch),
                  "channelizer_ms_per_push": round(med(t_ch), 3), "demodulator_ms_per_push": round(med(t_fm), 3),
                  "demodulator_over_channelizer": round(med(t_fm) / med(t_ch), 3), "source_sha": sha})
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
