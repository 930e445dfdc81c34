#!/bin/bash
# Evidence of one GPU: the GPU tests, the full bench line, the encoder and latency benches, and the per-kernel
# durations of the one-batch-in-flight bench under rocprofv3.  Usage: tools/evidence_run.sh OUT_DIR
set -e
mkdir -p "${1:?usage: tools/evidence_run.sh OUT_DIR}"
ev=$(cd "$1" && pwd)
export TMPDIR=${TMPDIR:-/tmp}
cd "$(dirname "$0")/.."
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$ev/pytest_gpu.log" 2>&1 || { tail -30 "$ev/pytest_gpu.log"; exit 1; }
tail -3 "$ev/pytest_gpu.log"
timeout -k 10 400 python bench.py --full > "$ev/bench.json" 2> "$ev/bench.err"
echo bench done
timeout -k 10 300 python tools/bench_encode.py --texts > "$ev/bench_encode.json" 2> "$ev/bench_encode.err"
echo encode done
timeout -k 10 300 python tools/bench_latency.py > "$ev/latency.json" 2> "$ev/latency.err"
echo latency done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$ev/prof_s1" -o s1 -- python3 bench.py --steps 100 --warmup 10 --streams 1 --full --no-cpu-baseline --no-check > "$ev/bench_s1_profiled.json" 2> "$ev/bench_s1.err"
echo prof done
