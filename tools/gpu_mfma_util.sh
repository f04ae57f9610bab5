#!/bin/bash
# MFMA utilisation (PMC) of the Schur / factorisation kernels on the headline configuration: its own rocprofv3 pass (counters only)
set -o pipefail
mkdir -p gpurun_out/prof_r05 profiles gpurun_out/profiles_r05
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
tmp=$(mktemp -d)
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d "$tmp/pmc_mfma" -- python3 bench.py --full --steps 20 --warmup 3 --probe 0 --no-cpu --no-parity --no-dense-leg --no-dense-relmeas --ingest-only --no-place-leg > "$tmp/pmc_mfma.log" 2>&1 || { tail -5 "$tmp/pmc_mfma.log"; exit 1; }
python3 tools/pmc_mfma_summary.py "$tmp/pmc_mfma" r05
cp profiles/r05_pmc_mfma_util.* gpurun_out/profiles_r05/
rm -rf "$tmp"
