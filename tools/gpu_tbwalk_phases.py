"""Where a k_p1_tbwalk wave's time goes INSIDE the 256-stream batch pass: shader cycles of every wave between the marks of
viterbi3_traceback_walk, summed (diagnostic build: python -m nrsc5_amd.build --tbwalk-phases  ->  nrsc5_amd/libnrsc5hip_tbphases.so).
python tools/gpu_tbwalk_phases.py [--lib OTHER_BUILD.so] [bench.py arguments]
--lib: a diagnostic build of another source tree (an A/B measurement: the freshness check is skipped, with a notice)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
extra = [a for a in sys.argv[1:]]
if "--lib" in extra:
    k = extra.index("--lib")
    os.environ["NRSC5HIP_AB_LIB"] = os.path.abspath(extra[k + 1])
    del extra[k:k + 2]
import torch
from nrsc5_amd import engine as _eng
if "NRSC5HIP_AB_LIB" not in os.environ:
    _eng.DEFAULT_LIB = os.path.join(ROOT, "nrsc5_amd", "libnrsc5hip_tbphases.so")
import bench
sys.argv = ["bench.py", "--no-cpu-baseline"] + extra
args = bench.parse()
dev = torch.device("cuda", 0)
W = bench.Fm(args, dev, 0, list(range(256)))
W.E.tune(_eng.TUNE_SYNC_PHASES, 1)
W.one_pass()
c0 = W.E.debug_sync_phases()
t0 = W.E.tb_stats()
steps, _ = W.one_pass()
c1 = W.E.debug_sync_phases()
t1 = W.E.tb_stats()
d = (c1 - c0)[8:11].astype(float)
ntasks = (t1[0] - t0[0]) / 2284.0 * 36                          # frames decoded in the pass x 36 waves each
names = ["staging (+ received signs)", "run-in + walk, stores", "re-encode count"]
for nm, v in zip(names, d):
    print(f"{nm:30s} {v / ntasks:9.0f} cycles per wave   {100.0 * v / d.sum():5.1f} %")
print(f"{'total':30s} {d.sum() / ntasks:9.0f} cycles per wave; {ntasks:.0f} waves; {steps} steps; chunks re-walked {t1[1] - t0[1]}; library {_eng.DEFAULT_LIB}; extra args {extra}")
