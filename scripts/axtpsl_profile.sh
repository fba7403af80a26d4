#!/bin/bash
# axtToPsl on lastz-like axt (profiles/axttopsl/):
#   sweep.txt         per input size: wall time of bin/axtToPsl -host (16 threads)
#                     and -device (device bring-up included), two runs each,
#                     alternating; the outputs compared byte for byte
#   tool_laps.txt     at the lap size: the stage laps of one -host and one -device
#                     run (-verbose=2, GAC_TIMING: the device call synchronises
#                     after every step, so its upload and kernel laps stand alone)
#   kernel_stats.csv  one rocprofv3 --kernel-trace --stats run of the -device tool
#   reference.txt     oracle/_ref/axtToPsl (tests/golden/make_axtpsl_golden.py builds
#                     it) once on the smallest input, if it is there
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make`.  Inputs come from scripts/axtfilter_synth.py (seeded) and two
# sizes files that name its sequences.
#   scripts/axtpsl_profile.sh [OUTDIR] ["SIZES in MB"] [LAP SIZE in MB]
set -o pipefail
OUT=${1:-profiles/axttopsl}
SIZES=${2:-"64 256 1024 2048 4096"}
LAP_MB=${3:-2048}
TMP=${TMPDIR:-/tmp}
B=genomealignmenttools_amd/bin
export GAC_THREADS=16
mkdir -p "$OUT"
W=$(mktemp -d "$TMP/gac_axtpsl.XXXXXX")
trap 'rm -rf "$W"' EXIT
now() { date +%s.%N; }
secs() { awk "BEGIN{printf \"%.3f\", $2 - $1}"; }
awk 'BEGIN{for (k = 1; k <= 22; ++k) printf "chr%d\t250000000\n", k}' > "$W/t.sizes"
awk 'BEGIN{for (k = 0; k < 997; ++k) printf "scaffold%d\t250000000\n", k}' > "$W/q.sizes"

run() {  # run PATHOPT IN OUT -> seconds in $T
  local t0 t1
  t0=$(now)
  timeout -k 10 600 $B/axtToPsl "$1" "$2" "$W/t.sizes" "$W/q.sizes" "$3" 2> "$W/err.txt" || { tail -5 "$W/err.txt"; exit 1; }
  t1=$(now)
  T=$(secs "$t0" "$t1")
}

{
  echo "# bin/axtToPsl IN tSizes qSizes OUT; wall seconds, two runs each (host, device, host, device)"
  echo "# size_MB bytes records psl_bytes host_1 device_1 host_2 device_2 device_best/host_best"
} > "$OUT/sweep.txt"
first=1
for mb in $SIZES; do
  free_kb=$(df -Pk "$W" | awk 'NR==2{print $4}')
  if [ "$free_kb" -lt $((mb * 1024 * 2)) ]; then
    echo "# $mb MB: left out, $free_kb KB free in $TMP" >> "$OUT/sweep.txt"
    continue
  fi
  echo "size $mb MB ..."
  timeout -k 10 600 python3 scripts/axtfilter_synth.py "$W/in.axt" $((mb << 20)) 1234 || exit 1
  run -host "$W/in.axt" "$W/host.psl"; h1=$T
  run -device "$W/in.axt" "$W/dev.psl"; d1=$T
  cmp "$W/host.psl" "$W/dev.psl" || { echo "outputs differ at $mb MB"; exit 1; }
  run -host "$W/in.axt" "$W/host.psl"; h2=$T
  run -device "$W/in.axt" "$W/dev.psl"; d2=$T
  echo "$mb $(stat -c %s "$W/in.axt") $(wc -l < "$W/dev.psl") $(stat -c %s "$W/dev.psl") $h1 $d1 $h2 $d2 $(awk "BEGIN{h=($h1<$h2)?$h1:$h2; d=($d1<$d2)?$d1:$d2; printf \"%.2f\", d/h}")" >> "$OUT/sweep.txt"
  if [ -n "$first" ]; then
    first=
    if [ -x oracle/_ref/axtToPsl ]; then
      t0=$(now)
      timeout -k 10 900 oracle/_ref/axtToPsl "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/ref.psl" || exit 1
      t1=$(now)
      {
        echo "# oracle/_ref/axtToPsl (the reference's build, one thread), one run, on the $mb MB input"
        echo "input $(stat -c %s "$W/in.axt") bytes, $(wc -l < "$W/ref.psl") records"
        echo "reference (one run)      $(secs "$t0" "$t1") s"
        echo "bin/axtToPsl -host       $( [ "$(awk "BEGIN{print ($h1<$h2)}")" = 1 ] && echo $h1 || echo $h2) s (best of two)"
        cmp "$W/host.psl" "$W/ref.psl" && echo "outputs equal byte for byte"
      } > "$OUT/reference.txt" || exit 1
      rm -f "$W/ref.psl"
    else
      echo "# oracle/_ref/axtToPsl is not on this machine: the reference was not timed" > "$OUT/reference.txt"
    fi
  fi
  if [ "$mb" = "$LAP_MB" ]; then
    echo "laps at $mb MB ..."
    GAC_TIMING=1 timeout -k 10 600 $B/axtToPsl -host -verbose=2 "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/host.psl" 2> "$W/laps_host.txt" || { tail -5 "$W/laps_host.txt"; exit 1; }
    GAC_TIMING=1 timeout -k 10 600 $B/axtToPsl -device -verbose=2 "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/dev.psl" 2> "$W/laps_dev.txt" || { tail -5 "$W/laps_dev.txt"; exit 1; }
    {
      echo "# input: $(stat -c %s "$W/in.axt") bytes, $(wc -l < "$W/dev.psl") records; GAC_THREADS=$GAC_THREADS"
      echo "# ---- bin/axtToPsl -host"
      grep -v '^\[gac_par_output\]' "$W/laps_host.txt"
      echo "# ---- bin/axtToPsl -device"
      grep -v '^\[gac_par_output\]' "$W/laps_dev.txt"
    } > "$OUT/tool_laps.txt"
    echo "kernel trace at $mb MB ..."
    # (GAC_PROFILE_EXIT: the tool leaves through exit(), so that the profiler writes its files)
    GAC_PROFILE_EXIT=1 HSA_ENABLE_SDMA=0 timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$W/prof" -o axtpsl --output-format csv -- \
      genomealignmenttools_amd/libexec/axtToPsl -device "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/prof.psl" > "$W/prof.log" 2>&1 \
      || { tail -20 "$W/prof.log"; exit 1; }
    cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
    rm -f "$W/prof.psl"
  fi
  rm -f "$W/in.axt" "$W/host.psl" "$W/dev.psl"
done
cat "$OUT/sweep.txt"
