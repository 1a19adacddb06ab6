#!/bin/bash
# Round 6: everything behind profiles/r06_* in one GPU call (repo root on the GPU box).
# usage: tools/r6_profiles.sh <outdir, relative to the repo root>
OUT=${1:?usage: tools/r6_profiles.sh <outdir>}
mkdir -p "$OUT"
for WL in swinir_x8 edsr_x8; do
  bash tools/refresh_profiles.sh $WL "$OUT/prof_$WL" > "$OUT/r6_refresh_$WL.log" 2>&1
  bash tools/step_mfma_pmc.sh "$OUT/mfma_$WL" $WL > "$OUT/r6_mfma_$WL.log" 2>&1
done
python bench.py --full > "$OUT/r6_bench_default.json" 2> "$OUT/r6_bench_default.err"
tail -c 400 "$OUT/r6_bench_default.json"
