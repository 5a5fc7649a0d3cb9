"""Cost of watching the analog hosts for EAS alerts (SAME, nrsc5hip_fm_same_*) in a WidebandReceiver session, and proof that the sessions without
it are untouched.  Three legs, one JSON line each per K:
    session    the scene of tools/gpu_analog_bench.py (K hybrid-FM stations with a stereo host in a 20 MS/s cs16 band), the same session two
               ways, --reps times each, alternating:
                   analog       analog=True
                   analog_eas   analog=True, eas=True
               wall time per session and per push, the medians, and what SAME adds.  The hosts carry no burst: the tone sums and the
               decisions cost the same on any input, and the framer is at its dearest while it searches (every bit position against 0xAB 0xAB).
    stage      the demodulator alone on the channelizer's output (FmDemod.process_tensor), without and with SAME: wall time per push, the
               medians -- the four SAME kernels next to the four audio kernels.
    untouched  the programs=True session and the analog=True session, --reps times each, in a child process per tree: this one, and with
               --ab-tree a checkout of the parent commit (its nrsc5_amd package with its library built), in the order A B B A A B B A (--rounds 4) behind one
               child of each tree that is not counted (the first child of a visit ran 3 % slower than the same tree's second: with
               A B A B and this tree in front the order was what got measured).  `pass` says whether the medians differ by no more than
               the spread between the parent's own repeats.
`python tools/gpu_same_bench.py [--k 8,32] [--frames 4] [--ab-tree DIR] [--out profiles/wideband_same.jsonl]`"""
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
    """-> per push, ms of the demodulator alone without SAME and with it"""
    import torch
    from nrsc5_amd import engine as eng
    n = cap.raw.numel() // 2
    ch = eng.Channelizer(cap.rate, eng.IQ_CS16, offs)
    plain, same = eng.FmDemod(len(offs)), eng.FmDemod(len(offs), same=True)
    t_off, t_on = [], []
    for p in range(0, n, chunk):
        y = ch.process_tensor(cap.raw[2 * p:2 * min(n, p + chunk)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.process_tensor(y)
        t1 = time.perf_counter()
        same.process_tensor(y)
        t2 = time.perf_counter()
        if min(n, p + chunk) - p == chunk and p:                     # whole pushes behind the first (its launches load the code objects)
            t_off.append(1e3 * (t1 - t0))
            t_on.append(1e3 * (t2 - t1))
    bits = same.same_stats(0)["bits"]
    ch.close(); plain.close(); same.close()
    return t_off, t_on, bits


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
    ap.add_argument("--rounds", type=int, default=4, help="untouched leg with --ab-tree: child processes per tree (a child's repeats lie closer together than two children's medians)")
    ap.add_argument("--legs", default="session,stage,untouched")
    ap.add_argument("--ab-tree", default=None, help="untouched leg: a checkout of the parent commit, library built, to run the same sessions with")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--child-untouched", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_untouched:
        return child_untouched(a)
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
                line[label] = {"wall_s": walls, "median_s": med(walls), "spread": round(max(walls) / min(walls), 4), "source_sha": runs[t][0]["source_sha"]}
            if a.ab_tree:
                ratio = line["this_tree"]["median_s"] / line["ab_tree"]["median_s"]
                line["this_tree_over_ab_tree"] = round(ratio, 4)
                line["order"] = "warm-up of each tree, then " + " ".join("A B" if r % 2 == 0 else "B A" for r in range(a.rounds))
                line["pass"] = bool(max(ratio, 1 / ratio) <= line["ab_tree"]["spread"])
            emit(line)
    if "session" not in a.legs and "stage" not in a.legs:
        return
    import torch
    torch.cuda.init()
    from nrsc5_amd import engine as eng
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for k in [int(v) for v in a.k.split(",")]:
        cap, offs = ab.scene(k, a.rate, a.frames, hosts=True)
        n = cap.raw.numel() // 2
        pushes = -(-n // a.chunk)
        if "session" in a.legs:
            modes = {"analog": {"analog": True}, "analog_eas": {"analog": True, "eas": True}}
            for m in modes:
                ab.session(cap, offs, a.chunk, **modes[m])               # warm-up: first launches, staging buffers
            wall = {m: [] for m in modes}
            for rep in range(a.reps):
                for m in modes:
                    wall[m].append(ab.session(cap, offs, a.chunk, **modes[m])[0])
            emit({"metric": "wideband_same_session", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes": pushes, "session_signal_s": round(n / a.rate, 2),
                  "sessions": a.reps, "session_wall_s": {m: [round(v, 4) for v in wall[m]] for m in modes},
                  "median_s": {m: round(med(wall[m]), 4) for m in modes},
                  "push_wall_ms": {m: round(1e3 * med(wall[m]) / pushes, 3) for m in modes},
                  "spread_of_repeats": {m: round(max(wall[m]) / min(wall[m]), 4) for m in modes},
                  "added_by_eas_s": round(med(wall["analog_eas"]) - med(wall["analog"]), 4),
                  "added_by_eas_share": round(med(wall["analog_eas"]) / med(wall["analog"]) - 1, 4), "source_sha": sha})
        if "stage" in a.legs:
            t_off, t_on, bits = stage(cap, offs, a.chunk)
            emit({"metric": "wideband_same_stage", "rate": a.rate, "channels": k, "chunk": a.chunk, "pushes_timed": len(t_off),
                  "demodulator_ms_per_push": round(med(t_off), 3), "demodulator_with_same_ms_per_push": round(med(t_on), 3),
                  "same_kernels_ms_per_push": round(med(t_on) - med(t_off), 3), "same_over_audio": round(med(t_on) / med(t_off) - 1, 3),
                  "bits_per_station": bits, "source_sha": sha})
        del cap
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
