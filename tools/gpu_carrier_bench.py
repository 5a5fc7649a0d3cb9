"""Cost of the carrier measurement (nrsc5hip_fm_carrier*) and of the scan for analog-only stations, and proof that the sessions without them are
untouched.  One JSON line per leg and K:
    session    the scene of tools/gpu_analog_bench.py (K hybrid-FM stations with a stereo host in a 20 MS/s cs16 band), the same session two
               ways, --reps times each, alternating:
                   analog           analog=True
                   analog_carrier   analog=True, carrier=True
               wall time per session and per push, the medians, and what the measurement adds.
    stage      the demodulator alone on the channelizer's output (FmDemod.process_tensor), without and with the measurement: wall time per
               push, the medians.
    untouched  the programs=True session and the analog=True session in a child process per tree (tools/gpu_rds_bench.py's child): this tree,
               and with --ab-tree a checkout of the parent commit with its library built, alternating A B A B.  `pass` says whether the medians
               differ by no more than the spread between the parent's own repeats.
    scan       wideband.scan() of a scene with two of the K stations analog-only, without and with analog=True, --reps times each, alternating;
               and the session at all K found centres against the session at the K - 2 HD centres alone: what two analog-only stations cost
               while they ride an engine stream that never locks.
`python tools/gpu_carrier_bench.py [--k 8,32] [--frames 4] [--ab-tree DIR] [--out profiles/wideband_carrier.jsonl]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import gpu_analog_bench as ab                                       # noqa: E402  (scene and session are that tool's)


def stage(cap, offs, chunk):
    """-> per push, ms of the demodulator alone without the measurement and with it"""
    import torch
    from nrsc5_amd import engine as eng
    n = cap.raw.numel() // 2
    ch = eng.Channelizer(cap.rate, eng.IQ_CS16, offs)
    plain, car = eng.FmDemod(len(offs)), eng.FmDemod(len(offs), carrier=True)
    t_off, t_on = [], []
    for p in range(0, n, chunk):
        y = ch.process_tensor(cap.raw[2 * p:2 * min(n, p + chunk)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.process_tensor(y)
        t1 = time.perf_counter()
        car.process_tensor(y)
        t2 = time.perf_counter()
        if min(n, p + chunk) - p == chunk and p:                     # whole pushes behind the first (its launches load the code objects)
            t_off.append(1e3 * (t1 - t0))
            t_on.append(1e3 * (t2 - t1))
    cnr = car.carrier()[0]["running"]["cnr_db"]
    ch.close(); plain.close(); car.close()
    return t_off, t_on, cnr


def analog_scene(k: int, rate: int, frames: int):
    """the scene of gpu_analog_bench.scene with stations 1 and k - 2 analog-only, on a 400 kHz raster: at 200 kHz a neighbour's host lies on a
    station's sidebands and nothing decodes, which a session at given centres does not mind and a scan does"""
    import numpy as np
    import torch
    from nrsc5_amd import synth_wideband as sw
    edge = rate / 2 - 198.5e3
    offs = [float(v) for v in np.clip((np.arange(k) - k // 2) * 400e3, -edge, edge)]
    rng = np.random.default_rng(k)
    st = [sw.Station(offset_hz=o, seed=900 + i, cfo_hz=float(rng.uniform(-3000, 3000)), timing=int(rng.integers(0, 4320)), host=ab.HOST, host_db=ab.HOST_DB,
                     digital=i not in (1, k - 2)) for i, o in enumerate(offs)]
    cap = sw.capture(st, rate, "cs16", n_frames=frames, noise_rms=0.02, rms_total=6000.0, seed=k, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return cap, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--frames", type=int, default=4, help="L1 frames per station (1.486 s each)")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--legs", default="session,stage,untouched,scan")
    ap.add_argument("--ab-tree", default=None, help="untouched leg: a checkout of the parent commit, library built, to run the same sessions with")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    if "untouched" in a.legs:
        k = int(a.k.split(",")[0])
        trees = [None] + ([os.path.abspath(a.ab_tree)] if a.ab_tree else [])
        runs = {t: [] for t in trees}
        for rnd in range(2 if a.ab_tree else 1):                     # A B A B: a fresh child process per run
            for t in trees:
                env = dict(os.environ)
                env.pop("NRSC5_BENCH_TREE", None)
                if t:
                    env["NRSC5_BENCH_TREE"] = t
                cmd = [sys.executable, os.path.join(ROOT, "tools", "gpu_rds_bench.py"), "--child-untouched", "--rate", str(a.rate), "--k", str(k),
                       "--frames", str(a.frames), "--chunk", str(a.chunk), "--reps", str(a.reps)]
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, timeout=1500)
                if r.returncode != 0:
                    raise SystemExit("untouched child failed: " + r.stderr.decode()[-2000:])
                runs[t].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        for name in ("programs", "analog"):
            line = {"metric": "wideband_%s_session_untouched" % name, "rate": a.rate, "channels": k, "chunk": a.chunk, "frames": a.frames}
            for t, label in zip(trees, ("this_tree", "ab_tree")):
                walls = [w for run in runs[t] for w in run[name]]
                line[label] = {"wall_s": walls, "median_s": med(walls), "spread": round(max(walls) / min(walls), 4), "source_sha": runs[t][0]["source_sha"]}
            if a.ab_tree:
                ratio = line["this_tree"]["median_s"] / line["ab_tree"]["median_s"]
                line["this_tree_over_ab_tree"] = round(ratio, 4)
                line["pass"] = bool(max(ratio, 1 / ratio) <= line["ab_tree"]["spread"])
            emit(line)
    if not {"session", "stage", "scan"} & set(a.legs.split(",")):
        return
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng, wideband
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for k in [int(v) for v in a.k.split(",")]:
        if "session" in a.legs or "stage" in a.legs:
            cap, offs = ab.scene(k, a.rate, a.frames, hosts=True)
            n = cap.raw.numel() // 2
            pushes = -(-n // a.chunk)
        if "session" in a.legs:
            modes = {"analog": {"analog": True}, "analog_carrier": {"analog": True, "carrier": True}}
            for m in modes:
                ab.session(cap, offs, a.chunk, **modes[m])               # warm-up: first launches, staging buffers
            wall = {m: [] for m in modes}
            for rep in range(a.reps):
                for m in modes:
                    wall[m].append(ab.session(cap, offs, a.chunk, **modes[m])[0])
            emit({"metric": "wideband_carrier_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": pushes, "session_signal_s": round(n / a.rate, 2),
                  "sessions": a.reps, "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes},
                  "median_s": {m: round(med(wall[m]), 4) for m in modes},
                  "push_wall_ms": {m: round(1e3 * med(wall[m]) / pushes, 3) for m in modes},
                  "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes},
                  "added_by_carrier_s": round(med(wall["analog_carrier"]) - med(wall["analog"]), 4),
                  "added_by_carrier_share": round(med(wall["analog_carrier"]) / med(wall["analog"]) - 1, 4), "source_sha": sha})
        if "stage" in a.legs:
            t_off, t_on, cnr = stage(cap, offs, a.chunk)
            emit({"metric": "wideband_carrier_stage", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes_timed": len(t_off),
                  "demodulator_ms_per_push": round(med(t_off), 3), "demodulator_with_carrier_ms_per_push": round(med(t_on), 3),
                  "carrier_ms_per_push": round(med(t_on) - med(t_off), 3), "carrier_over_audio": round(med(t_on) / med(t_off) - 1, 3),
                  "running_cnr_db_station0": round(cnr, 2), "source_sha": sha})
        if "session" in a.legs or "stage" in a.legs:
            del cap
            torch.cuda.empty_cache()
        if "scan" in a.legs:
            cap, offs = analog_scene(k, a.rate, a.frames)
            n = cap.raw.numel() // 2
            wall = {False: [], True: []}
            found = {}
            for rep in range(a.reps + 1):                                # the first pair is the warm-up
                for on in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    found[on] = wideband.scan(cap.raw, cap.rate, cap.fmt, analog=on)
                    torch.cuda.synchronize()
                    if rep:
                        wall[on].append(time.perf_counter() - t0)
            kinds = [s.kind for s in found[True]]
            emit({"metric": "wideband_scan_analog", "rate": a.rate, "stations": k, "analog_only": 2, "scan_wall_s": {"hd": [round(v, 4) for v in wall[False]],
                  "hd_and_analog": [round(v, 4) for v in wall[True]]}, "median_s": {"hd": round(med(wall[False]), 4), "hd_and_analog": round(med(wall[True]), 4)},
                  "found": {"hd": len(found[False]), "hd_and_analog": len(found[True]), "analog": kinds.count("analog")}, "source_sha": sha})
            hd = [s.offset_hz for s in found[True] if s.kind == "hd"]
            both = [s.offset_hz for s in found[True]]
            if not hd or len(both) == len(hd):
                raise SystemExit("the scan found %d HD and %d analog-only stations: nothing to compare" % (len(hd), len(both) - len(hd)))
            ab.session(cap, both, a.chunk, analog=True)
            ride = {"hd": [], "hd_and_analog": []}
            for rep in range(a.reps):
                ride["hd"].append(ab.session(cap, hd, a.chunk, analog=True)[0])
                ride["hd_and_analog"].append(ab.session(cap, both, a.chunk, analog=True)[0])
            emit({"metric": "wideband_analog_only_on_engine_streams", "rate": a.rate, "hd_stations": len(hd), "analog_only": len(both) - len(hd),
                  "pushes": -(-n // a.chunk), "session_wall_s": {m: [round(v, 4) for v in ride[m]] for m in ride},
                  "median_s": {m: round(med(ride[m]), 4) for m in ride},
                  "added_per_analog_only_station_s": round((med(ride["hd_and_analog"]) - med(ride["hd"])) / max(1, len(both) - len(hd)), 4), "source_sha": sha})
            del cap
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
