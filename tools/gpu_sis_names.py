"""How long a band scan has to decode before it can name a station: the first-name time of every station of the band-scan scenes A, B and D
(tests/scan_model.py: 2.4 MS/s cu8 and 10 MS/s cs16, stations of unequal level, one under an analog host), each transmitting a SIS schedule
(tests/sis_args.py) that starts at another place of its cycle, so that the name is not the first thing every receiver sees.  The capture is
pushed in --step seconds through wideband.confirm_stations(names=True); a station's time is the capture time at the end of the push whose SIS
snapshot first holds a name.  One JSON line per scene; wideband.NAME_SECONDS is twice the largest time.
`python tools/gpu_sis_names.py [--frames 5] [--out profiles/wideband_sis_names.jsonl]`"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    import torch
    from nrsc5_amd import channel, engine as eng, synth_wideband as sw, wideband
    from tests import sis_args as sa
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5, help="L1 frames per station (1.486 s each)")
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = eng.load_library().nrsc5hip_source_sha().decode()

    def pids(k):
        fr = sa.schedule(k % 3, never_complete=False)
        return np.roll(fr, -((23 * k) % len(fr)), axis=0)
    scenes = {
        "A": (2400000, "cu8", dict(noise_rms=0.02, seed=3),
              [sw.Station(offset_hz=o, seed=500 + k, level=l, pids=pids(k)) for k, (o, l) in enumerate(zip([-800e3, 0.0, 600e3], [1.0, 0.6, 0.8]))]),
        "B": (10000000, "cs16", dict(noise_rms=0.05, rms_total=6000.0, seed=8),
              [sw.Station(offset_hz=o, seed=300 + k, cfo_hz=1000.0 * (k - 3), level=l, chan=channel.Impairments(host_db=20.0) if k == 5 else None, pids=pids(k))
               for k, (o, l) in enumerate(zip([-4.6e6, -3.0e6, -1.8e6, -1.6e6, 0.4e6, 1.2e6, 2.8e6, 4.4e6], [1.0, 0.7, 1.0, 0.1, 0.5, 0.8, 1.0, 0.6]))]),
        "D": (10000000, "cs16", dict(noise_rms=0.4, seed=4),
              [sw.Station(offset_hz=o, seed=900 + k, level=l, pids=pids(k)) for k, (o, l) in enumerate(zip([-3e6, -1e6, 1e6, 3e6], [1.0, 0.5, 0.25, 0.125]))]),
    }
    worst = 0.0
    for name, (rate, fmt, kw, st) in scenes.items():
        cap = sw.capture(st, rate, fmt, n_frames=a.frames, device=dev, **kw)
        seconds = cap.raw.numel() / 2 / rate
        found = [wideband.FoundStation(s.offset_hz - s.cfo_hz, 10.0, 0.0, 0.0) for s in st]
        kept = wideband.confirm_stations(cap.raw, rate, fmt, found, chunk=int(a.step * rate), names=True, name_seconds=seconds)
        times = [s.first_name_s for s in kept]
        line = {"metric": "wideband_first_name", "scene": name, "rate": rate, "format": fmt, "stations": len(st), "confirmed": len(kept), "capture_s": round(seconds, 2),
                "step_s": a.step, "first_pids_s": [s.first_pids_s for s in kept], "first_name_s": times, "names": [s.name for s in kept],
                "largest_first_name_s": max(t for t in times if t is not None) if any(t is not None for t in times) else None, "unnamed": sum(t is None for t in times),
                "source_sha": sha}
        if line["largest_first_name_s"]:
            worst = max(worst, line["largest_first_name_s"])
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del cap
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "wideband_first_name", "largest_first_name_s": worst, "name_seconds": round(2 * worst, 2)}), flush=True)


if __name__ == "__main__":
    main()
