"""Speed of the band scan's spectrum survey (nrsc5hip_scan_push): a 20.8 s capture synthesised on the device, 20 MS/s cs16 at the
default nfft (8192) and 2.4 MS/s cu8 (2048), pushed in one call.  nrsc5hip_scan_push runs on the scanner's own stream and returns when
it is done, so `wall_s` is the host time of that blocking call (launches and the wait included; best of --reps after a warm-up);
kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.  Prints one JSON line per case: x real time of
the capture and the algorithmic HBM bytes (the input, once) over wall_s as a fraction of the MI355X's 8 TB/s.
`python tools/gpu_scan_bench.py [--seconds S] [--reps N] [--chunk SAMPLES]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # B/s


def main():
    import torch
    from nrsc5_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, help="samples per push (0: the whole capture in one push)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sha = eng.load_library().nrsc5hip_source_sha().decode()
    for rate, fmt in ((20000000, "cs16"), (2400000, "cu8")):
        n = int(a.seconds * rate)
        if fmt == "cs16":
            x = torch.clamp(torch.randn(2 * n, generator=g, device=dev) * 3000, -32768, 32767).to(torch.int16)
        else:
            x = torch.clamp(127 + torch.randn(2 * n, generator=g, device=dev) * 40, 0, 255).to(torch.uint8)
        torch.cuda.synchronize()
        sc = eng.Scanner(rate, eng.IQ_FORMATS[fmt])
        chunk = a.chunk or n
        times = []
        for r in range(a.reps + 1):
            sc.reset()
            t0 = time.perf_counter()
            for p in range(0, n, chunk):
                sc.push(x.data_ptr() + p * 2 * x.element_size(), min(chunk, n - p))      # returns when the scanner's stream is done
            if r:
                times.append(time.perf_counter() - t0)
        s = min(times)
        psd = sc.spectrum()[1]
        bytes_moved = 2 * x.element_size() * n
        print(json.dumps({"metric": "band_scan_survey", "rate": rate, "format": fmt, "capture_s": a.seconds, "nfft": sc.nfft,
                          "segments": sc.segments, "pushes": -(-n // chunk), "wall_s": round(s, 5), "wall_s_all": [round(t, 5) for t in times],
                          "x_realtime": round(a.seconds / s, 1), "input_bytes": bytes_moved, "hbm_fraction": round(bytes_moved / s / HBM_PEAK, 4),
                          "mean_psd": float(psd.mean()), "source_sha": sha}), flush=True)
        sc.close()
        del x


if __name__ == "__main__":
    main()
