#!/bin/bash
# chainToPsl on C5 (profiles/chaintopsl/): k_psl_counts beside
# k_compose on the whole chain set -- wall times, alternated with a library
# variant of an earlier commit when one is given (k_compose shares its walk
# with k_psl_counts; `make variant NAME=parent VSRC=<that commit's csrc>`) --
# then one rocprofv3 --kernel-trace --stats run, then the tool's own stage
# laps (GAC_TIMING), twice.  Needs `make all synth`.
#   scripts/chaintopsl_profile.sh [OUTDIR] [VARIANT]
set -o pipefail
OUT=${1:-profiles/chaintopsl}
VAR=${2:-}
TMP=${TMPDIR:-/tmp}
D=$TMP/gac_bench_c5_5000000_1234   # bench.py's C5 directory
mkdir -p "$OUT"
if [ ! -f "$D/info.json" ]; then
  timeout -k 10 200 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains=5000000 \
    -sizesDir=genomealignmenttools_amd/data -threads=16 || exit 1
fi
W=$(mktemp -d)
: > "$OUT/prof_psl.json"
for k in 1 2; do
  if [ -n "$VAR" ]; then
    GAC_LIB_VARIANT=$VAR timeout -k 10 240 python scripts/chaintopsl_profile.py "$D" > "$W/run.log" 2>&1 \
      || { tail -20 "$W/run.log"; exit 1; }
    grep PROF_JSON "$W/run.log" | sed 's/^PROF_JSON //' >> "$OUT/prof_psl.json"
  fi
  timeout -k 10 240 python scripts/chaintopsl_profile.py "$D" > "$W/run.log" 2>&1 \
    || { tail -20 "$W/run.log"; exit 1; }
  grep PROF_JSON "$W/run.log" | sed 's/^PROF_JSON //' >> "$OUT/prof_psl.json"
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$W" -o c5 --output-format csv -- \
  python scripts/chaintopsl_profile.py "$D" > "$W/run.log" 2>&1 || { tail -20 "$W/run.log"; exit 1; }
cp "$(find "$W" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
: > "$OUT/tool_laps.txt"
for k in 1 2; do
  echo "== run $k" >> "$OUT/tool_laps.txt"
  GAC_TIMING=1 timeout -k 10 400 genomealignmenttools_amd/bin/chainToPsl "$D/in.chain" "$W/no.t.sizes" \
    "$W/no.q.sizes" "$D/t.2bit" "$D/q.2bit" "$W/out.psl" 2>> "$OUT/tool_laps.txt" || exit 1
done
echo "$(wc -l < "$W/out.psl") lines, $(stat -c %s "$W/out.psl") bytes, sha256 $(sha256sum "$W/out.psl" | cut -c1-16)" >> "$OUT/tool_laps.txt"
rm -rf "$W"
