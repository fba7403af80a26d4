#!/bin/bash
# A/B of the four sequence tools on C5 (profiles/seqtool/): an
# earlier build's bin/ directory against this tree's, alternating, three runs
# each of chainAntiRepeat, chainToPsl, netToAxt (on the T net bin/chainNet makes)
# and chainToAxt.  Per run: wall time, the output stage's lap (GAC_TIMING),
# sha256 and size of the output; the stage laps of each side's first run go to
# ab_laps.txt.  Every step runs under its own timeout; a failing step ends the
# script.  Needs `make all synth` in both trees.
#   scripts/seqtool_ab.sh PARENT_BIN_DIR [OUTDIR]
set -o pipefail
PARENT=${1:?usage: scripts/seqtool_ab.sh PARENT_BIN_DIR [OUTDIR]}
OUTDIR=${2:-profiles/seqtool}
mkdir -p "$OUTDIR"
OUT=$OUTDIR/ab.txt
LAPS=$OUTDIR/ab_laps.txt
TMP=${TMPDIR:-/tmp}
D=$TMP/gac_bench_c5_5000000_1234   # bench.py's C5 directory
W=$(mktemp -d)
: > $OUT
if [ ! -f "$D/info.json" ]; then
  timeout -k 10 300 genomealignmenttools_amd/libexec/gac_synth c5 "$D" -seed=1234 -chains=5000000 \
    -sizesDir=genomealignmenttools_amd/data -threads=16 > $W/synth.log 2>&1 || { tail -5 $W/synth.log; exit 1; }
fi
echo "# synth done $(date +%T)" >> $OUT
timeout -k 10 300 $PARENT/chainNet "$D/in.chain" "$D/t.sizes" "$D/q.sizes" \
  "$W/t.net" /dev/null > "$W/chainnet.log" 2>&1 || { tail -5 "$W/chainnet.log"; exit 1; }
echo "# chainNet done $(date +%T): $(grep -c '^net' $W/t.net) nets" >> $OUT
echo "# tool side run wall_s lap_s sha256 (lap: the 'render + write output' / 'write output' stage)" >> $OUT

one() { # tool side run
  local tool=$1 side=$2 run=$3 B=genomealignmenttools_amd/bin o=$W/out
  [ $side = parent ] && B=$PARENT
  local -a cmd
  case $tool in
    chainAntiRepeat) cmd=($B/chainAntiRepeat "$D/t.2bit" "$D/q.2bit" "$D/in.chain" $o);;
    chainToAxt) cmd=($B/chainToAxt "$D/in.chain" "$D/t.2bit" "$D/q.2bit" $o);;
    netToAxt) cmd=($B/netToAxt "$W/t.net" "$D/in.chain" "$D/t.2bit" "$D/q.2bit" $o);;
    chainToPsl) cmd=($B/chainToPsl "$D/in.chain" "$W/no.t.sizes" "$W/no.q.sizes" "$D/t.2bit" "$D/q.2bit" $o);;
  esac
  rm -f $o
  local t0=$(date +%s.%N)
  GAC_TIMING=1 timeout -k 10 300 "${cmd[@]}" -verbose=2 2> $W/laps.txt || { echo "$tool $side failed: $?"; tail -5 $W/laps.txt; return 1; }
  local t1=$(date +%s.%N)
  local lap=$(grep -E '\[stage\] (render \+ write output|write output) ' $W/laps.txt | sed -E 's/.*output +([0-9.]+) s.*/\1/')
  local sha=$(sha256sum $o | cut -c1-16)
  echo "$tool $side $run $(awk "BEGIN{printf \"%.3f\", $t1 - $t0}") $lap $sha $(stat -c %s $o)" | tee -a $OUT
  if [ $run = 1 ]; then { echo "## $tool $side laps"; grep -v '^Processing ' $W/laps.txt | grep -E 'stage\]|chainToAxt\]|netToAxt\]|batches' | sed 's/^/#   /'; } >> $LAPS; fi
  rm -f $o
}

: > $LAPS
for tool in chainAntiRepeat chainToPsl netToAxt chainToAxt; do
  for run in 1 2 3; do
    one $tool parent $run && one $tool tree $run || exit 1
  done
done
rm -rf $W
echo "# done $(date +%T)" >> $OUT
# per tool: medians, the parent's own spread as the margin, outputs equal
python3 - "$OUT" >> $OUT <<'PY'
import statistics, sys
rows = [ln.split() for ln in open(sys.argv[1]) if ln[0] != "#"]
for tool in dict.fromkeys(r[0] for r in rows):
    wall = {s: [float(r[3]) for r in rows if r[0] == tool and r[1] == s] for s in ("parent", "tree")}
    sha = {r[5] for r in rows if r[0] == tool}
    mp, mt = statistics.median(wall["parent"]), statistics.median(wall["tree"])
    spread = max(wall["parent"]) - min(wall["parent"])
    print(f"# {tool}: parent median {mp:.3f} s (max - min {spread:.3f} s), tree median {mt:.3f} s: "
          f"{'within' if mt <= mp + spread else 'OVER'} parent + spread; "
          f"{'one sha256 ' + sha.pop() if len(sha) == 1 else 'OUTPUTS DIFFER'}")
PY
