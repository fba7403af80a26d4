#!/bin/bash
# chainPreNet on C5 (profiles/prenet/): bin/chainPreNet on the
# whole C5 chain file with its stage laps (GAC_TIMING) on the device and with
# -host, one rocprofv3 --kernel-trace --stats run of the tool for the kernel
# times, and one timed run of the reference binary on the same file.  The
# outputs' sha256 go into tool_laps.txt.
# Every step runs under its own timeout; a failing step ends the script.
# Needs `make all synth`, and for the reference its binary, compiled as
# tests/golden/make_prenet_golden.py compiles it (GAC_REF_PRENET=path, default
# oracle/_ref/chainPreNet; without it the reference is left out and said so).
#   scripts/prenet_profile.sh [OUTDIR] [seconds allowed to the reference]
set -o pipefail
OUT=${1:-profiles/prenet}
REF_LIMIT=${2:-600}
REF_BIN=${GAC_REF_PRENET:-oracle/_ref/chainPreNet}
TMP=${TMPDIR:-/tmp}
D=$TMP/gac_bench_c5_5000000_1234   # bench.py's C5 directory
B=genomealignmenttools_amd/bin
mkdir -p "$OUT"
W=$(mktemp -d)
if [ ! -f "$D/info.json" ]; then
  timeout -k 10 200 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains=5000000 \
    -sizesDir=genomealignmenttools_amd/data -threads=16 || exit 1
fi
echo "chainPreNet (device) ..."
GAC_TIMING=1 timeout -k 10 300 $B/chainPreNet "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/dev.chain" -verbose=2 \
  2> "$W/laps_dev.txt" || { tail -5 "$W/laps_dev.txt"; exit 1; }
echo "chainPreNet -host ..."
GAC_TIMING=1 timeout -k 10 300 $B/chainPreNet -host "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/host.chain" -verbose=2 \
  2> "$W/laps_host.txt" || { tail -5 "$W/laps_host.txt"; exit 1; }
{
  echo "# input: $(grep -c '^chain' "$D/in.chain") chains, $(stat -c %s "$D/in.chain") bytes; kept $(grep -c '^chain' "$W/dev.chain")"
  echo "# ---- bin/chainPreNet (device)"
  grep -v '^\[gt_read_chains\]' "$W/laps_dev.txt"
  echo "# ---- bin/chainPreNet -host"
  grep -v '^\[gt_read_chains\]' "$W/laps_host.txt"
} > "$OUT/tool_laps.txt"
echo "kernel trace ..."
# (GAC_PROFILE_EXIT: the tool leaves through exit(), so that the profiler writes its files)
GAC_PROFILE_EXIT=1 HSA_ENABLE_SDMA=0 timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$W/prof" -o c5 --output-format csv -- \
  genomealignmenttools_amd/libexec/chainPreNet "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/prof.chain" > "$W/prof.log" 2>&1 \
  || { tail -20 "$W/prof.log"; exit 1; }
cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats.csv"
{
  if [ -x "$REF_BIN" ]; then
    echo "reference (at most $REF_LIMIT s) ..." >&2
    t0=$(date +%s.%N)
    timeout -k 10 "$REF_LIMIT" "$REF_BIN" "$D/in.chain" "$D/t.sizes" "$D/q.sizes" "$W/ref.chain" 2> "$W/ref.err"
    rc=$?
    t1=$(date +%s.%N)
    echo "# ---- the reference chainPreNet (one run)"
    if [ $rc -eq 0 ]; then
      echo "reference wall $(awk "BEGIN{printf \"%.2f\", $t1 - $t0}") s"
      echo "sha256 reference $(sha256sum "$W/ref.chain" | cut -d' ' -f1)"
    else
      echo "reference did not finish: exit status $rc after $(awk "BEGIN{printf \"%.2f\", $t1 - $t0}") s (limit $REF_LIMIT s)"
    fi
  else
    echo "# ---- the reference chainPreNet: $REF_BIN not built, left out"
  fi
  echo "sha256 device    $(sha256sum "$W/dev.chain" | cut -d' ' -f1)"
  echo "sha256 host      $(sha256sum "$W/host.chain" | cut -d' ' -f1)"
  echo "sha256 profiled  $(sha256sum "$W/prof.chain" | cut -d' ' -f1)"
} >> "$OUT/tool_laps.txt"
rm -rf "$W"
