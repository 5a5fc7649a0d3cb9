"""Cost of the reception impairments (multipath and adjacent-channel detectors, nrsc5hip_fm_impair*) in a WidebandReceiver session, and proof that
the sessions without them are untouched.  Four legs, one JSON line each per K:
    session    the scene of tools/gpu_analog_bench.py (K hybrid-FM stations with a stereo host in a 20 MS/s cs16 band), the same session two
               ways, --reps times each, alternating:
                   analog_carrier          analog=True, carrier=True
                   analog_carrier_impair   analog=True, carrier=True, impair=True
               wall time per session and per push, the medians, and what the detectors add (the feature's own cost: reported, not gated).
    stage      the demodulator alone on the channelizer's output (FmDemod.process_tensor) with the carrier measurement, without and with the
               detectors: wall time per push, the medians -- the two impairment kernels next to the audio and carrier kernels.
    untouched  the programs=True session and the analog=True session, --reps times each, in a child process per tree: this one, and with
               --ab-tree a checkout of the parent commit (its nrsc5_amd package with its library built), in the order A B B A .. (--rounds) behind
               one child of each tree that is not counted.  `pass` says whether the medians differ by no more than the spread between the
               parent's own repeats.
    bench      with --ab-tree: `bench.py --gpus 1 --steps S --warmup W --no-cpu-baseline --no-extra-legs` in either tree, A B B A, the same gate.
`python tools/gpu_impair_bench.py [--k 8,32] [--frames 4] [--ab-tree DIR] [--out profiles/wideband_impair.jsonl]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NRSC5_BENCH_TREE") or ROOT)      # (the untouched leg's child: the package of the tree it measures)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import gpu_analog_bench as ab                                       # noqa: E402  (scene and session are that tool's)


def stage(cap, offs, chunk):
    """-> per push, ms of the demodulator with the carrier measurement alone and with the detectors on top; station 0's last windowed report"""
    import torch
    from nrsc5_amd import engine as eng
    n = cap.raw.numel() // 2
    ch = eng.Channelizer(cap.rate, eng.IQ_CS16, offs)
    car, imp = eng.FmDemod(len(offs), carrier=True), eng.FmDemod(len(offs), impair=True)
    t_car, t_imp, last = [], [], None
    for p in range(0, n, chunk):
        y = ch.process_tensor(cap.raw[2 * p:2 * min(n, p + chunk)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        car.process_tensor(y)
        t1 = time.perf_counter()
        imp.process_tensor(y)
        t2 = time.perf_counter()
        if min(n, p + chunk) - p == chunk and p:                     # whole pushes behind the first (its launches load the code objects)
            t_car.append(1e3 * (t1 - t0))
            t_imp.append(1e3 * (t2 - t1))
        if p // chunk == n // chunk // 2:                            # in the middle of the session: the capture runs on behind the end of the transmissions
            last = imp.impair()[0]["windowed"]
    ch.close(); car.close(); imp.close()
    return t_car, t_imp, last


def child_untouched(a):
    """one tree (the one this process imports): the programs and the analog session a.reps times each behind a warm-up; prints the wall times as JSON"""
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng
    k = int(a.k.split(",")[0])
    out = {"source_sha": eng.load_library().nrsc5hip_source_sha().decode()}
    cap, offs = ab.scene(k, a.rate, a.frames, hosts=True)
    for name, kw in (("programs", dict(programs=True)), ("analog", dict(analog=True))):
        ab.session(cap, offs, a.chunk, **kw)
        out[name] = [round(ab.session(cap, offs, a.chunk, **kw)[0], 4) for _ in range(a.reps)]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--frames", type=int, default=4, help="L1 frames per station (1.486 s each)")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3, help="repeats of each session")
    ap.add_argument("--rounds", type=int, default=2, help="untouched and bench legs with --ab-tree: child processes per tree")
    ap.add_argument("--legs", default="session,stage,untouched,bench")
    ap.add_argument("--ab-tree", default=None, help="untouched and bench legs: a checkout of the parent commit, library built")
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--child-untouched", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_untouched:
        return child_untouched(a)
    med = lambda v: sorted(v)[len(v) // 2]
    legs = set(a.legs.split(","))

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def verdict(line):
        if a.ab_tree:
            ratio = line["this_tree"]["median"] / line["ab_tree"]["median"]
            line["this_tree_over_ab_tree"] = round(ratio, 4)
            line["order"] = "warm-up of each tree, then " + " ".join("A B" if r % 2 == 0 else "B A" for r in range(a.rounds))
            line["pass"] = bool(max(ratio, 1 / ratio) <= line["ab_tree"]["spread"])
        emit(line)

    trees = [None] + ([os.path.abspath(a.ab_tree)] if a.ab_tree else [])
    if "untouched" in legs:
        k = int(a.k.split(",")[0])
        runs = {t: [] for t in trees}

        def run_child(t):
            env = dict(os.environ)
            env.pop("NRSC5_BENCH_TREE", None)
            if t:
                env["NRSC5_BENCH_TREE"] = t
            cmd = [sys.executable, os.path.abspath(__file__), "--child-untouched", "--rate", str(a.rate), "--k", str(k), "--frames", str(a.frames),
                   "--chunk", str(a.chunk), "--reps", str(a.reps)]
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, timeout=1500)
            if r.returncode != 0:
                raise SystemExit("untouched child failed: " + r.stderr.decode()[-2000:])
            return json.loads(r.stdout.decode().strip().splitlines()[-1])

        if a.ab_tree:                                                # a child of each tree that is not counted: whichever runs first on an idle device is the slower
            for t in reversed(trees):
                run_child(t)
        for rnd in range(a.rounds if a.ab_tree else 1):              # A B B A ..: a fresh child process per run, neither tree always in front
            for t in (trees if rnd % 2 == 0 else trees[::-1]):
                runs[t].append(run_child(t))
        for name in ("programs", "analog"):
            line = {"metric": "wideband_%s_session_untouched" % name, "rate": a.rate, "channels": k, "chunk": a.chunk, "frames": a.frames}
            for t, label in zip(trees, ("this_tree", "ab_tree")):
                walls = [w for run in runs[t] for w in run[name]]
                line[label] = {"wall_s": walls, "median": med(walls), "spread": round(max(walls) / min(walls), 4), "source_sha": runs[t][0]["source_sha"]}
            verdict(line)
    if "bench" in legs and a.ab_tree:
        vals = {t: [] for t in trees}
        key = None

        def run_bench(t):
            nonlocal key
            cwd = t or ROOT
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline", "--no-extra-legs"]
            r = subprocess.run(cmd, cwd=cwd, capture_output=True, timeout=1500)
            if r.returncode != 0:
                raise SystemExit("bench.py failed in %s: %s" % (cwd, r.stderr.decode()[-2000:]))
            res = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
            key = key or next(n for n in ("value", "primary", "streams_realtime", "x_realtime") if n in res)
            print("# bench.py in %s: %s %s" % (cwd, key, res[key]), file=sys.stderr, flush=True)
            return float(res[key])

        for rnd in range(a.rounds):
            for t in (trees if rnd % 2 == 0 else trees[::-1]):
                vals[t].append(run_bench(t))
        line = {"metric": "bench_py_untouched", "field": key, "steps": a.bench_steps, "warmup": a.bench_warmup}
        for t, label in zip(trees, ("this_tree", "ab_tree")):
            line[label] = {"values": vals[t], "median": med(vals[t]), "spread": round(max(vals[t]) / min(vals[t]), 4)}
        verdict(line)
    if not {"session", "stage"} & legs:
        return
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for k in [int(v) for v in a.k.split(",")]:
        cap, offs = ab.scene(k, a.rate, a.frames, hosts=True)
        n = cap.raw.numel() // 2
        pushes = -(-n // a.chunk)
        if "session" in legs:
            modes = {"analog_carrier": {"analog": True, "carrier": True}, "analog_carrier_impair": {"analog": True, "carrier": True, "impair": True}}
            for m in modes:
                ab.session(cap, offs, a.chunk, **modes[m])               # warm-up: first launches, staging buffers
            wall = {m: [] for m in modes}
            for rep in range(a.reps):
                for m in modes:
                    wall[m].append(ab.session(cap, offs, a.chunk, **modes[m])[0])
            emit({"metric": "wideband_impair_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": pushes, "session_signal_s": round(n / a.rate, 2),
                  "sessions": a.reps, "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes},
                  "median_s": {m: round(med(wall[m]), 4) for m in modes},
                  "push_wall_ms": {m: round(1e3 * med(wall[m]) / pushes, 3) for m in modes},
                  "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes},
                  "added_by_impair_s": round(med(wall["analog_carrier_impair"]) - med(wall["analog_carrier"]), 4),
                  "added_by_impair_share": round(med(wall["analog_carrier_impair"]) / med(wall["analog_carrier"]) - 1, 4), "source_sha": sha})
        if "stage" in legs:
            t_car, t_imp, last = stage(cap, offs, a.chunk)
            emit({"metric": "wideband_impair_stage", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes_timed": len(t_car),
                  "demodulator_with_carrier_ms_per_push": round(med(t_car), 3), "demodulator_with_impair_ms_per_push": round(med(t_imp), 3),
                  "impair_kernels_ms_per_push": round(med(t_imp) - med(t_car), 3), "impair_over_carrier": round(med(t_imp) / med(t_car) - 1, 3),
                  "station0": {q: (round(v, 4) if isinstance(v, float) else v) for q, v in (last or {}).items() if q in
                               ("explained", "depth", "rho", "usn_db", "ripple_db", "multipath", "adjacent", "side")}, "source_sha": sha})
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
