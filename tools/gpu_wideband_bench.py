"""Speed of the wideband channelizer (nrsc5hip_chan_process): a 20.8 s, 20 MS/s cs16 capture synthesised on the device, K channels
on the 200 kHz grid.  nrsc5hip_chan_process runs on the channelizer's own stream and returns when it is done, so `wall_s` is the host
time of that blocking call (launches and the wait included; best of --reps after a warm-up); kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool.  Prints one JSON line per K: x real time of the capture, channel-seconds per
second, algorithmic HBM bytes (input once, outputs once) and FP32 FMAs against the MI355X peaks, and for comparison the engine's batch
time (nrsc5hip_batch_append_cs16 + nrsc5hip_batch_process, p1_async, l2_feedback) on the same K channelized streams.
`python tools/gpu_wideband_bench.py [--seconds S] [--k 8,32,64,128] [--no-engine]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # B/s
FP32_PEAK = 157.3e12       # FLOP/s, unpacked vector rate


def main():
    import numpy as np
    import torch
    from nrsc5_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.8)
    ap.add_argument("--rate", type=int, default=20000000)
    ap.add_argument("--k", default="8,32,64,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(a.seconds * a.rate)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.clamp(torch.randn(2 * n, generator=g, device=dev) * 3000, -32768, 32767).to(torch.int16)
    torch.cuda.synchronize()
    for k in [int(v) for v in a.k.split(",")]:
        edge = a.rate / 2 - 198.5e3
        offs = np.clip((np.arange(k) - k // 2) * 200e3, -edge, edge)
        ch = eng.Channelizer(a.rate, eng.IQ_CS16, offs)
        m = ch.outputs_for(n)
        out = torch.empty((k, m, 2), dtype=torch.int16, device=dev)
        times = []
        for r in range(a.reps + 1):
            ch.reset()
            t0 = time.perf_counter()
            ch.process(x.data_ptr(), n, out.data_ptr(), 2 * m, m)        # returns when the channelizer's stream is done
            if r:
                times.append(time.perf_counter() - t0)
        s = min(times)
        T = ch.taps
        bytes_moved = 4 * n + 4 * m * k                                  # cs16 in, cs16 out, each once
        fmas = m * k * T * 2 + n * k * 4                                 # FIR (I and Q) + mixer
        print(json.dumps({"metric": "wideband_channelizer", "rate": a.rate, "capture_s": a.seconds, "channels": k, "taps": T,
                          "phases": ch.phases, "wall_s": round(s, 5), "x_realtime": round(a.seconds / s, 1),
                          "channel_s_per_s": round(a.seconds * k / s, 1), "hbm_fraction": round(bytes_moved / s / HBM_PEAK, 4),
                          "fp32_fraction": round(2 * fmas / s / FP32_PEAK, 4), "source_sha": eng.load_library().nrsc5hip_source_sha().decode()}),
              flush=True)
        ch.close()
        if not a.no_engine:
            E = eng.Engine(max_streams=k, q15_capacity=m + 64, record_capacity=512, p1_slots=int(a.seconds / 1.486) + 12, p1_async=True,
                           l2_feedback=True)
            E.batch_append_cs16(out.data_ptr(), 2 * m, [2 * m] * k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.batch_process(k)
            E.batch_fetch(k, with_frames=False)
            te = time.perf_counter() - t0
            E.close()
            print(json.dumps({"metric": "engine_batch_same_streams", "channels": k, "capture_s": a.seconds, "wall_s": round(te, 4),
                              "x_realtime": round(a.seconds / te, 1), "note": "append (untimed) + batch_process + batch_fetch of the K channelized streams"}),
                  flush=True)
        del out


if __name__ == "__main__":
    main()
