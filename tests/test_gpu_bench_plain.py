"""`-m gpu`: a plain `bench.py` run (no --full) times the headline only -- its line carries the headline fields and none of the checks --
and two runs with the same arguments write the same --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


def _plain(out):
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "bench.py"), "--streams", "16", "--seconds", "5", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_gpu_plain_bench_line_and_repeatable_outputs(hip_lib, tmp_path):
    a, b = _plain(tmp_path / "a"), _plain(tmp_path / "b")
    for line in (a, b):
        assert line["metric"] == "IQ MS/s demod+decoded" and line["unit"] == "IQ MS/s" and line["higher_is_better"] is True and line["dtype"]
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["full"] is False and line["parity"] is None and line["cpu_baseline"] is None and line["parity_failures"] == []
        assert not any(k in line for k in ("single_stream", "in_order", "dropin", "config4"))
    fa, fb = sorted(os.listdir(tmp_path / "a")), sorted(os.listdir(tmp_path / "b"))
    assert fa == fb and "counts.npy" in fa and "frame_words.npy" in fa
    for f in fa:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert np.load(tmp_path / "a" / "counts.npy").sum() > 0 and np.load(tmp_path / "a" / "frame_index.npy").shape[0] > 0
