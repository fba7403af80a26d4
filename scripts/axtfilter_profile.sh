#!/bin/bash
# filterAxtIdentityEntropy.py on lastz-like axt (profiles/axtfilter/):
#   sweep.txt         per input size: wall time of bin/filterAxtIdentityEntropy.py
#                     -host (16 threads) and -device (device bring-up included),
#                     two runs each, alternating; the outputs compared byte for byte
#   tool_laps.txt     at the lap size: the stage laps of one -host and one -device
#                     run (-verbose=2, GAC_TIMING: the device call synchronises
#                     after every step, so its upload and kernel laps stand alone)
#   kernel_stats.csv  one rocprofv3 --kernel-trace --stats run of the -device tool
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make`.  Inputs come from scripts/axtfilter_synth.py (seeded).
#   scripts/axtfilter_profile.sh [OUTDIR] ["SIZES in MB"] [LAP SIZE in MB]
set -o pipefail
OUT=${1:-profiles/axtfilter}
SIZES=${2:-"64 256 1024 2048 4096"}
LAP_MB=${3:-2048}
ARGS="60 1.8 30"   # minSeqIdent minEntropy windowSize
TMP=${TMPDIR:-/tmp}
B=genomealignmenttools_amd/bin
export GAC_THREADS=16
mkdir -p "$OUT"
W=$(mktemp -d "$TMP/gac_axtf.XXXXXX")
trap 'rm -rf "$W"' EXIT
now() { date +%s.%N; }
secs() { awk "BEGIN{printf \"%.3f\", $2 - $1}"; }

run() {  # run PATHOPT IN OUT -> seconds in $T
  local t0 t1
  t0=$(now)
  timeout -k 10 600 $B/filterAxtIdentityEntropy.py "$1" "$2" $ARGS "$3" 2> "$W/err.txt" || { tail -5 "$W/err.txt"; exit 1; }
  t1=$(now)
  T=$(secs "$t0" "$t1")
}

{
  echo "# bin/filterAxtIdentityEntropy.py IN $ARGS OUT; wall seconds, two runs each (host, device, host, device)"
  echo "# size_MB bytes entries kept host_1 device_1 host_2 device_2 device_best/host_best"
} > "$OUT/sweep.txt"
for mb in $SIZES; do
  free_kb=$(df -Pk "$W" | awk 'NR==2{print $4}')
  if [ "$free_kb" -lt $((mb * 1024 * 7 / 2)) ]; then
    echo "# $mb MB: left out, $free_kb KB free in $TMP" >> "$OUT/sweep.txt"
    continue
  fi
  echo "size $mb MB ..."
  timeout -k 10 600 python3 scripts/axtfilter_synth.py "$W/in.axt" $((mb << 20)) 1234 || exit 1
  run -host "$W/in.axt" "$W/host.axt"; h1=$T
  run -device "$W/in.axt" "$W/dev.axt"; d1=$T
  cmp "$W/host.axt" "$W/dev.axt" || { echo "outputs differ at $mb MB"; exit 1; }
  run -host "$W/in.axt" "$W/host.axt"; h2=$T
  run -device "$W/in.axt" "$W/dev.axt"; d2=$T
  echo "$mb $(stat -c %s "$W/in.axt") $(grep -c '^[0-9]' "$W/in.axt") $(grep -c '^[0-9]' "$W/dev.axt") $h1 $d1 $h2 $d2 $(awk "BEGIN{h=($h1<$h2)?$h1:$h2; d=($d1<$d2)?$d1:$d2; printf \"%.2f\", d/h}")" >> "$OUT/sweep.txt"
  if [ "$mb" = "$LAP_MB" ]; then
    echo "laps at $mb MB ..."
    GAC_TIMING=1 timeout -k 10 600 $B/filterAxtIdentityEntropy.py -host -verbose=2 "$W/in.axt" $ARGS "$W/host.axt" 2> "$W/laps_host.txt" || { tail -5 "$W/laps_host.txt"; exit 1; }
    GAC_TIMING=1 timeout -k 10 600 $B/filterAxtIdentityEntropy.py -device -verbose=2 "$W/in.axt" $ARGS "$W/dev.axt" 2> "$W/laps_dev.txt" || { tail -5 "$W/laps_dev.txt"; exit 1; }
    {
      echo "# input: $(stat -c %s "$W/in.axt") bytes, $(grep -c '^[0-9]' "$W/in.axt") entries; arguments $ARGS; GAC_THREADS=$GAC_THREADS"
      echo "# ---- bin/filterAxtIdentityEntropy.py -host"
      grep -v '^\[gac_par_output\]' "$W/laps_host.txt"
      echo "# ---- bin/filterAxtIdentityEntropy.py -device"
      grep -v '^\[gac_par_output\]' "$W/laps_dev.txt"
    } > "$OUT/tool_laps.txt"
    echo "kernel trace at $mb MB ..."
    # (GAC_PROFILE_EXIT: the tool leaves through exit(), so that the profiler writes its files)
    GAC_PROFILE_EXIT=1 HSA_ENABLE_SDMA=0 timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$W/prof" -o axtf --output-format csv -- \
      genomealignmenttools_amd/libexec/filterAxtIdentityEntropy.py -device "$W/in.axt" $ARGS "$W/prof.axt" > "$W/prof.log" 2>&1 \
      || { tail -20 "$W/prof.log"; exit 1; }
    cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
    rm -f "$W/prof.axt"
  fi
  rm -f "$W/in.axt" "$W/host.axt" "$W/dev.axt"
done
cat "$OUT/sweep.txt"
