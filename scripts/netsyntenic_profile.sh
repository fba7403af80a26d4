#!/bin/bash
# netSyntenic on C5 (profiles/netsyntenic/): bin/chainNet once
# for the T net, its "net" lines without fills dropped (the reference refuses
# them, tests/golden/make_netfilter_golden.py), then bin/netSyntenic on it with
# its stage laps (GAC_TIMING) on the device and with -host, one rocprofv3
# --kernel-trace --stats run of the tool for the kernel times, and one timed
# run of the reference binary (oracle/_ref/netSyntenic) on the same file.  The
# three outputs' sha256 go into tool_laps.txt.
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make all synth ref`.
#   scripts/netsyntenic_profile.sh [OUTDIR] [seconds allowed to the reference]
set -o pipefail
OUT=${1:-profiles/netsyntenic}
REF_LIMIT=${2:-600}
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
timeout -k 10 200 $B/chainNet "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/raw.net" /dev/null \
  > "$W/chainnet.log" 2>&1 || { tail -5 "$W/chainnet.log"; exit 1; }
# a "net" line that no indented line follows has no fills
awk '/^net /{ if (held != "") dropped++; held = $0; next }
     { if (held != "" && /^ /) print held; else if (held != "") dropped++; held = ""; print }
     END { if (held != "") dropped++; print dropped + 0 > "/dev/stderr" }' "$W/raw.net" > "$W/t.net" 2> "$W/dropped.txt"
rm -f "$W/raw.net"
echo "netSyntenic (device) ..."
GAC_TIMING=1 timeout -k 10 240 $B/netSyntenic "$W/t.net" "$W/dev.net" -verbose=2 2> "$W/laps_dev.txt" \
  || { tail -5 "$W/laps_dev.txt"; exit 1; }
echo "netSyntenic -host ..."
GAC_TIMING=1 timeout -k 10 240 $B/netSyntenic -host "$W/t.net" "$W/host.net" -verbose=2 2> "$W/laps_host.txt" \
  || { tail -5 "$W/laps_host.txt"; exit 1; }
{
  echo "# input: $(grep -c '^net' "$W/t.net") nets ($(cat "$W/dropped.txt") without fills dropped), $(grep -c ' fill ' "$W/t.net") fills, $(grep -c ' gap ' "$W/t.net") gaps, $(stat -c %s "$W/t.net") bytes"
  echo "# ---- bin/netSyntenic (device)"
  cat "$W/laps_dev.txt"
  echo "# ---- bin/netSyntenic -host"
  cat "$W/laps_host.txt"
} > "$OUT/tool_laps.txt"
echo "kernel trace ..."
# (GAC_PROFILE_EXIT: the tool leaves through exit(), so that the profiler writes its files)
GAC_PROFILE_EXIT=1 HSA_ENABLE_SDMA=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$W/prof" -o c5 --output-format csv -- \
  genomealignmenttools_amd/libexec/netSyntenic "$W/t.net" "$W/prof.net" > "$W/prof.log" 2>&1 \
  || { tail -20 "$W/prof.log"; exit 1; }
cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
echo "reference (at most $REF_LIMIT s) ..."
t0=$(date +%s.%N)
timeout -k 10 "$REF_LIMIT" oracle/_ref/netSyntenic "$W/t.net" "$W/ref.net" 2> "$W/ref.err"
rc=$?
t1=$(date +%s.%N)
{
  echo "# ---- oracle/_ref/netSyntenic (one run)"
  if [ $rc -eq 0 ]; then
    echo "reference wall $(awk "BEGIN{printf \"%.2f\", $t1 - $t0}") s; $(cat "$W/ref.err")"
    echo "sha256 reference $(sha256sum "$W/ref.net" | cut -d' ' -f1)"
  else
    echo "reference did not finish: exit status $rc after $(awk "BEGIN{printf \"%.2f\", $t1 - $t0}") s (limit $REF_LIMIT s)"
  fi
  echo "sha256 device    $(sha256sum "$W/dev.net" | cut -d' ' -f1)"
  echo "sha256 host      $(sha256sum "$W/host.net" | cut -d' ' -f1)"
  echo "sha256 profiled  $(sha256sum "$W/prof.net" | cut -d' ' -f1)"
} >> "$OUT/tool_laps.txt"
rm -rf "$W"
