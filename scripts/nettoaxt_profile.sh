#!/bin/bash
# netToAxt on C5 (profiles/nettoaxt/): bin/chainNet once for the
# T net, bin/netToAxt on it with its stage laps (GAC_TIMING), then one
# rocprofv3 --kernel-trace --stats run of the cut kernels and of k_axt_stat /
# k_axt_render in clip mode beside the unclipped kernels on the same pieces.
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make all synth`.
#   scripts/nettoaxt_profile.sh [OUTDIR]
set -o pipefail
OUT=${1:-profiles/nettoaxt}
TMP=${TMPDIR:-/tmp}
D=$TMP/gac_bench_c5_5000000_1234   # bench.py's C5 directory
B=genomealignmenttools_amd/bin
mkdir -p "$OUT"
W=$(mktemp -d)
if [ ! -f "$D/info.json" ]; then
  timeout -k 10 200 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains=5000000 \
    -sizesDir=genomealignmenttools_amd/data -threads=16 || exit 1
fi
echo "chainNet ..."
timeout -k 10 200 $B/chainNet "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/t.net" /dev/null \
  > "$W/chainnet.log" 2>&1 || { tail -5 "$W/chainnet.log"; exit 1; }
echo "netToAxt ..."
GAC_TIMING=1 timeout -k 10 240 $B/netToAxt "$W/t.net" "$D/in.chain" "$D/t.2bit" "$D/q.2bit" "$W/out.axt" \
  -verbose=2 2> "$W/laps.txt" || { tail -5 "$W/laps.txt"; exit 1; }
grep -v '^Processing ' "$W/laps.txt" > "$OUT/tool_laps.txt"   # (one line per net, as the reference prints)
echo "net: $(grep -c '^net' "$W/t.net") nets, $(grep -c ' id ' "$W/t.net") fills; wrote $(stat -c %s "$W/out.axt") bytes, $(grep -c '^[0-9]' "$W/out.axt") records, sha256 $(sha256sum "$W/out.axt" | cut -c1-16)" >> "$OUT/tool_laps.txt"
rm -f "$W/out.axt"
echo "kernel trace ..."
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$W" -o c5 --output-format csv -- \
  python scripts/nettoaxt_profile.py "$D" > "$W/run.log" 2>&1 || { tail -20 "$W/run.log"; exit 1; }
grep PROF_JSON "$W/run.log" | sed 's/^PROF_JSON //' > "$OUT/prof_netaxt.json"
cp "$(find "$W" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
rm -rf "$W"
