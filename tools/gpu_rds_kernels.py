"""Per-kernel times of the analog FM demodulator with RDS: K channels (argument, default 8), 30 pushes of 156 066 samples (one push of 4 194 304
samples at 20 MS/s, channelized) of a noisy carrier each.  Run it under the profiler, in a run of its own:
`rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/gpu_rds_kernels.py 8`; the figures are in profiles/wideband_rds_kernels.txt."""
import os
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nrsc5_amd import engine as eng
K = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = 156066
rng = np.random.default_rng(K)
ph = np.cumsum(rng.uniform(-0.6, 0.6, (K, n)), axis=1)
x = np.stack([8000 * np.cos(ph), 8000 * np.sin(ph)], axis=2) + rng.normal(0, 100, (K, n, 2))
x = torch.from_numpy(np.rint(x).astype(np.int16)).cuda()
D = eng.FmDemod(K, rds=True)
for _ in range(30):
    D.process_tensor(x)
print("launches", D.launches(), "bits", D.rds_stats(0)["bits"])
D.close()
