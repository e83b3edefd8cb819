#!/usr/bin/env bash
# A/B of the 1-bit fused middle step: table-driven (default) vs per-element tree (BAGUA_ONEBIT_LUT=0)
#   bash tools/ab_onebit_lut.sh OUT_DIR
set -euo pipefail
OUT=${1:?usage: ab_onebit_lut.sh OUT_DIR}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread -p no:cacheprovider \
  -k "onebit or OneBit or rccl_procs" > "$OUT/tests.log" 2>&1
for r in 1 2; do
  BAGUA_ONEBIT_LUT=0 timeout -k 10 200 python3 tools/onebit_reduce_probe.py > "$OUT/probe_off_$r.json"
  timeout -k 10 200 python3 tools/onebit_reduce_probe.py > "$OUT/probe_on_$r.json"
done
timeout -k 10 200 python3 tools/onebit_reduce_probe.py --dtype bf16 > "$OUT/probe_on_bf16.json"
AR=(bench.py --full --workload allreduce --no-decentralized)  # the 1-bit side line (onebit_allreduce) needs --full
for r in 1 2; do
  BAGUA_ONEBIT_LUT=0 timeout -k 10 200 python3 "${AR[@]}" > "$OUT/ar1_off_$r.json"
  timeout -k 10 200 python3 "${AR[@]}" > "$OUT/ar1_on_$r.json"
done
