#!/bin/bash
# the default bench and the round's profiles
set -o pipefail
mkdir -p gpurun_out
err=$(mktemp)
timeout -k 10 600 python bench.py --full > profiles/r04_bench_default.json 2> "$err" || { echo "bench failed"; tail -5 "$err"; exit 1; }
echo "bench done"
timeout -k 10 900 bash tools/profile_round.sh r04 || { echo "profile failed"; exit 1; }
echo "profiles done"
