#!/bin/bash
# the whole GPU suite on the tree with the new defaults, then the default bench line
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p bench_logs; TAG=${1:-r06f}
( time timeout 1800 python -m pytest tests -m gpu -q -s ) > bench_logs/${TAG}_tests.log 2>&1; echo "tests rc=$?"; grep -a "fuzz\|flow bursts\|passed\|failed\|^FAILED\|^ERROR" bench_logs/${TAG}_tests.log | cut -c1-500 | tail -14
( time timeout 900 python bench.py --full ) > bench_logs/${TAG}_bench.log 2>bench_logs/${TAG}_bench.err; echo "bench rc=$?"; tail -1 bench_logs/${TAG}_bench.log | cut -c1-600
