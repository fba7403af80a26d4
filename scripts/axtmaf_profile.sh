#!/bin/bash
# axtToMaf -score on lastz-like axt (profiles/axttomaf/):
#   sweep.txt         per input size: wall time of bin/axtToMaf -score -host (16
#                     threads) and -device (device bring-up included), two runs
#                     each, alternating; the outputs compared byte for byte
#   tool_laps.txt     at the lap size: the stage laps of one -host and one -device
#                     run (-verbose=2, GAC_TIMING: the device call synchronises
#                     after every step, so its upload and kernel laps stand alone)
#   kernel_stats.csv  one rocprofv3 --kernel-trace --stats run of the -device tool
#   kernel_rates.txt  at the lap size, on the same input in the same run: the
#                     "kernels" lap (GAC_TIMING) of gac_axt_score, gac_axt_psl and
#                     gac_axt_filter, in GB/s of uploaded text
#   reference.txt     oracle/_ref/axtToMaf and oracle/_ref/axtSort
#                     (tests/golden/make_axtmaf_golden.py builds them) once on the
#                     smallest input, if they are there
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make`.  Inputs come from scripts/axtfilter_synth.py (seeded) and two
# sizes files that name its sequences.
#   scripts/axtmaf_profile.sh [OUTDIR] ["SIZES in MB"] [LAP SIZE in MB]
set -o pipefail
OUT=${1:-profiles/axttomaf}
SIZES=${2:-"64 256 1024 2048 4096"}
LAP_MB=${3:-2048}
TMP=${TMPDIR:-/tmp}
B=genomealignmenttools_amd/bin
export GAC_THREADS=16
mkdir -p "$OUT"
W=$(mktemp -d "$TMP/gac_axtmaf.XXXXXX")
trap 'rm -rf "$W"' EXIT
now() { date +%s.%N; }
secs() { awk "BEGIN{printf \"%.3f\", $2 - $1}"; }
awk 'BEGIN{for (k = 1; k <= 22; ++k) printf "chr%d\t250000000\n", k}' > "$W/t.sizes"
awk 'BEGIN{for (k = 0; k < 997; ++k) printf "scaffold%d\t250000000\n", k}' > "$W/q.sizes"

run() {  # run PATHOPT IN OUT -> seconds in $T
  local t0 t1
  t0=$(now)
  timeout -k 10 600 $B/axtToMaf -score "$1" "$2" "$W/t.sizes" "$W/q.sizes" "$3" 2> "$W/err.txt" || { tail -5 "$W/err.txt"; exit 1; }
  t1=$(now)
  T=$(secs "$t0" "$t1")
}

{
  echo "# bin/axtToMaf -score IN tSizes qSizes OUT; wall seconds, two runs each (host, device, host, device)"
  echo "# size_MB bytes records maf_bytes host_1 device_1 host_2 device_2 device_best/host_best"
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
  run -host "$W/in.axt" "$W/host.maf"; h1=$T
  run -device "$W/in.axt" "$W/dev.maf"; d1=$T
  cmp "$W/host.maf" "$W/dev.maf" || { echo "outputs differ at $mb MB"; exit 1; }
  run -host "$W/in.axt" "$W/host.maf"; h2=$T
  run -device "$W/in.axt" "$W/dev.maf"; d2=$T
  echo "$mb $(stat -c %s "$W/in.axt") $(grep -c "^a " "$W/dev.maf") $(stat -c %s "$W/dev.maf") $h1 $d1 $h2 $d2 $(awk "BEGIN{h=($h1<$h2)?$h1:$h2; d=($d1<$d2)?$d1:$d2; printf \"%.2f\", d/h}")" >> "$OUT/sweep.txt"
  if [ -n "$first" ]; then
    first=
    if [ -x oracle/_ref/axtToMaf ] && [ -x oracle/_ref/axtSort ]; then
      t0=$(now)
      timeout -k 10 900 oracle/_ref/axtToMaf -score "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/ref.maf" || exit 1
      t1=$(now)
      timeout -k 10 900 oracle/_ref/axtSort "$W/in.axt" "$W/ref.axt" || exit 1
      t2=$(now)
      timeout -k 10 600 $B/axtSort "$W/in.axt" "$W/sorted.axt" || exit 1
      t3=$(now)
      {
        echo "# oracle/_ref/axtToMaf -score and oracle/_ref/axtSort (the reference's builds, one thread), one run each,"
        echo "# on the $mb MB input, on the same host in the same run as the sweep"
        echo "input $(stat -c %s "$W/in.axt") bytes, $(grep -c "^a " "$W/ref.maf") records"
        echo "reference axtToMaf -score (one run)  $(secs "$t0" "$t1") s"
        echo "bin/axtToMaf -score -host            $( [ "$(awk "BEGIN{print ($h1<$h2)}")" = 1 ] && echo $h1 || echo $h2) s (best of two)"
        cmp "$W/host.maf" "$W/ref.maf" && echo "axtToMaf: outputs equal byte for byte"
        echo "reference axtSort (one run)          $(secs "$t1" "$t2") s"
        echo "bin/axtSort (one run)                $(secs "$t2" "$t3") s"
        cmp "$W/sorted.axt" "$W/ref.axt" && echo "axtSort: outputs equal byte for byte"
      } > "$OUT/reference.txt" || exit 1
      rm -f "$W/ref.maf" "$W/ref.axt" "$W/sorted.axt"
    else
      echo "# oracle/_ref/axtToMaf and axtSort are not on this machine: the reference was not timed" > "$OUT/reference.txt"
    fi
  fi
  if [ "$mb" = "$LAP_MB" ]; then
    echo "laps at $mb MB ..."
    GAC_TIMING=1 timeout -k 10 600 $B/axtToMaf -score -host -verbose=2 "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/host.maf" 2> "$W/laps_host.txt" || { tail -5 "$W/laps_host.txt"; exit 1; }
    GAC_TIMING=1 timeout -k 10 600 $B/axtToMaf -score -device -verbose=2 "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/dev.maf" 2> "$W/laps_dev.txt" || { tail -5 "$W/laps_dev.txt"; exit 1; }
    {
      echo "# input: $(stat -c %s "$W/in.axt") bytes, $(grep -c "^a " "$W/dev.maf") records; GAC_THREADS=$GAC_THREADS"
      echo "# ---- bin/axtToMaf -score -host"
      grep -v '^\[gac_par_output\]' "$W/laps_host.txt"
      echo "# ---- bin/axtToMaf -score -device"
      grep -v '^\[gac_par_output\]' "$W/laps_dev.txt"
    } > "$OUT/tool_laps.txt"
    echo "kernel rates at $mb MB ..."
    GAC_TIMING=1 timeout -k 10 600 $B/axtToPsl -device "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/rate.psl" 2> "$W/rate_psl.txt" || { tail -5 "$W/rate_psl.txt"; exit 1; }
    GAC_TIMING=1 timeout -k 10 600 $B/filterAxtIdentityEntropy.py -device "$W/in.axt" 60 1.8 30 "$W/rate.axt" 2> "$W/rate_filter.txt" || { tail -5 "$W/rate_filter.txt"; exit 1; }
    {
      echo "# the kernels' lap of each call (GAC_TIMING: the stream is synchronised around it), -device,"
      echo "# on the same $(stat -c %s "$W/in.axt") bytes in the same run"
      grep -h ' kernels ' "$W/laps_dev.txt" "$W/rate_psl.txt" "$W/rate_filter.txt"
    } > "$OUT/kernel_rates.txt"
    rm -f "$W/rate.psl" "$W/rate.axt"
    echo "kernel trace at $mb MB ..."
    # (GAC_PROFILE_EXIT: the tool leaves through exit(), so that the profiler writes its files)
    GAC_PROFILE_EXIT=1 HSA_ENABLE_SDMA=0 timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$W/prof" -o axtmaf --output-format csv -- \
      genomealignmenttools_amd/libexec/axtToMaf -score -device "$W/in.axt" "$W/t.sizes" "$W/q.sizes" "$W/prof.maf" > "$W/prof.log" 2>&1 \
      || { tail -20 "$W/prof.log"; exit 1; }
    cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
    rm -f "$W/prof.maf"
  fi
  rm -f "$W/in.axt" "$W/host.maf" "$W/dev.maf"
done
cat "$OUT/sweep.txt"
