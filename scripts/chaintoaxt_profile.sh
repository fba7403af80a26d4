#!/bin/bash
# chainToAxt on C5 (profiles/chaintoaxt/): one rocprofv3
# --kernel-trace --stats run of k_axt_stat / k_axt_render beside k_compose on
# the same chains, then the tool's own stage laps (GAC_TIMING) on the whole
# chain file.  Needs `make all synth`.
#   scripts/chaintoaxt_profile.sh [OUTDIR]
set -o pipefail
OUT=${1:-profiles/chaintoaxt}
TMP=${TMPDIR:-/tmp}
D=$TMP/gac_bench_c5_5000000_1234   # bench.py's C5 directory
mkdir -p "$OUT"
if [ ! -f "$D/info.json" ]; then
  timeout -k 10 200 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains=5000000 \
    -sizesDir=genomealignmenttools_amd/data -threads=16 || exit 1
fi
W=$(mktemp -d)
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$W" -o c5 --output-format csv -- \
  python scripts/chaintoaxt_profile.py "$D" > "$W/run.log" 2>&1 || { tail -20 "$W/run.log"; exit 1; }
grep PROF_JSON "$W/run.log" | sed 's/^PROF_JSON //' > "$OUT/prof_axtout.json"
cp "$(find "$W" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
GAC_TIMING=1 timeout -k 10 240 genomealignmenttools_amd/bin/chainToAxt "$D/in.chain" "$D/t.2bit" \
  "$D/q.2bit" "$W/out.axt" -verbose=2 2> "$OUT/tool_laps.txt" || { tail -5 "$OUT/tool_laps.txt"; exit 1; }
echo "wrote $(stat -c %s "$W/out.axt") bytes, $(grep -c '^[0-9]' "$W/out.axt") records, sha256 $(sha256sum "$W/out.axt" | cut -c1-16)" >> "$OUT/tool_laps.txt"
rm -rf "$W"
