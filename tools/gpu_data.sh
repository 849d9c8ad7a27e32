#!/bin/bash
# Data-layer GPU session: parity tests, bench line, rocprof kernel stats.
set -o pipefail
export TMPDIR=/tmp
TAG=${1:-data}
mkdir -p gpurun_out
OUT=${ACN_OUT:-bench_out}; mkdir -p "$OUT"   # where the --full bench lines go
timeout -k 10 400 python -u -m pytest tests/test_data_gpu.py -v --timeout 120 --timeout-method thread -p no:cacheprovider > gpurun_out/pytest_$TAG.log 2>&1 \
&& timeout -k 10 300 python bench.py --full --workload data --cpu-seconds 10 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err \
&& timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof_$TAG -o run -- python3 bench.py --workload data --steps 20 --warmup 3 --no-cpu-baseline > gpurun_out/prof_$TAG.log 2>&1
echo "gpu_data exit=$?"
