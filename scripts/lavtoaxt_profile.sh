#!/bin/bash
# lavToAxt -host against -device end to end at several sizes, and k_axt_pairs
# beside k_axt_stat on the largest (profiles/lavtoaxt/).  The
# inputs are the pieces of gac_synth chain sets written as .lav.  Needs
# `make all synth`.  One time limit per step; a failing step ends the script.
#   scripts/lavtoaxt_profile.sh [OUTDIR] [chain counts ...]
set -o pipefail
OUT=${1:-profiles/lavtoaxt}
shift
SIZES=${*:-20000 100000 500000}
TMP=${TMPDIR:-/tmp}
BIN=genomealignmenttools_amd/bin/lavToAxt
mkdir -p "$OUT"
W=$(mktemp -d)
now() { date +%s.%N; }
: > "$OUT/e2e.txt"
for N in $SIZES; do
  D=$TMP/gac_lav_c5_${N}_1234
  if [ ! -f "$D/info.json" ]; then
    timeout -k 10 200 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains="$N" \
      -sizesDir=genomealignmenttools_amd/data -threads=16 > /dev/null || exit 1
  fi
  timeout -k 10 300 python scripts/lavtoaxt_profile.py lav "$D" "$W/in.lav" >> "$OUT/e2e.txt" || exit 1
  for rep in 1 2 3; do
    t0=$(now)
    timeout -k 10 300 $BIN -host "$W/in.lav" "$D/t.2bit" "$D/q.2bit" "$W/host.axt" || exit 1
    t1=$(now)
    timeout -k 10 300 $BIN -device "$W/in.lav" "$D/t.2bit" "$D/q.2bit" "$W/dev.axt" || exit 1
    t2=$(now)
    cmp "$W/host.axt" "$W/dev.axt" || exit 1
    echo "chains $N rep $rep: -host $(awk "BEGIN{printf \"%.3f\", $t1 - $t0}") s, -device $(awk "BEGIN{printf \"%.3f\", $t2 - $t1}") s," \
      "$(stat -c %s "$W/dev.axt") bytes of axt, equal" >> "$OUT/e2e.txt"
  done
  GAC_TIMING=1 timeout -k 10 300 $BIN -device "$W/in.lav" "$D/t.2bit" "$D/q.2bit" "$W/dev.axt" -verbose=2 \
    2> "$W/device_laps.txt" || exit 1
  GAC_TIMING=1 timeout -k 10 300 $BIN -host "$W/in.lav" "$D/t.2bit" "$D/q.2bit" "$W/host.axt" -verbose=2 \
    2> "$W/host_laps.txt" || exit 1
done
{ echo; echo "stage laps at $N chains (GAC_TIMING, -verbose=2), -host:"; grep '^\[stage\]' "$W/host_laps.txt"
  echo "-device:"; grep '^\[stage\]\|batches' "$W/device_laps.txt"; } >> "$OUT/e2e.txt"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$W/prof" -o pairs --output-format csv -- \
  python scripts/lavtoaxt_profile.py kernels "$D" > "$W/run.log" 2>&1 || { tail -20 "$W/run.log"; exit 1; }
grep PROF_JSON "$W/run.log" | sed 's/^PROF_JSON //' > "$OUT/prof_pairs.json"
cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
rm -rf "$W"
