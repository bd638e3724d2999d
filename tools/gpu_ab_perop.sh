#!/bin/bash
# same-box A/B of library variants: headline + the per-kernel averages of the persistent convolution.  tools/gpu_ab_perop.sh v1 v2 ...
cd "${GRAFT_REPO_ROOT:-/root/repo}"; mkdir -p gpurun_out
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for v in "$@"; do
  lib=libgtts_$v.so; [ "$v" = product ] && lib=libgradtts_gfx950.so
  GTTS_LIB=$PWD/speech-backbones_amd/$lib timeout 400 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --per-op > $OUT/v_$v.json 2> $OUT/v_$v.txt
  echo "== $v $(python -c "import json;d=json.load(open('$OUT/v_$v.json'));print(d['value'], d['config']['ms_per_unet_call'], d['config']['output_finite'])" 2>&1 | tail -1)"
  grep -E "^gtts::conv3x3_ws_kernel" $OUT/v_$v.txt | awk '{printf "   %s %s %s %s %s %s %s %s  launches %s avg %s\n", $1,$2,$3,$4,$5,$6,$7,$8,$9,$10}'
done
