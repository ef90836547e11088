#!/bin/bash
# usage (on the GPU box): tools/ab_alternate.sh <output directory> <variant.so> [pairs, default 3]
#   The tree's library and ONE variant build, alternating (tree, variant, tree, variant, ...) in one call on one box, so that the spread between two
#   runs of the SAME library is measured next to the difference between the two.  Per run: the one-stream stage times (bench.py --full --no-extras),
#   the default two-stream headline (bench.py) and the rocprofv3 per-kernel averages of the profiled one-stream form.  Every GPU step has a time limit
#   of its own and the first one that fails ends the call.  Results in the output directory, the table on stdout.
#   AB_KERNEL (default "k_idct_color<1>") and AB_STAGE (default idct_color) choose the kernel and the stage of the table,
#   e.g. AB_KERNEL="k_write2<7" AB_STAGE=write for the write pass (profiles/r09_second_symbol.txt).
set -o pipefail
mkdir -p "$1" || exit 1
OUT=$(realpath "$1"); VAR=$(realpath "$2"); PAIRS=${3:-3}
ROOT=$PWD; W=${TMPDIR:-/tmp}
LIB=$ROOT/jpegsnoop_amd/libjsnoop_gpu.so
TREE=$(mktemp "$W/libjsnoop_gpu.tree.XXXXXX.so")
cp "$LIB" "$TREE" || exit 1
trap 'cp "$TREE" "$LIB"; rm -f "$TREE"' EXIT
one() {   # name, library, run number
  local N=$1_$3
  cp "$2" "$LIB" &&
  timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --cpu-seconds 0 --no-extras 2>"$OUT/$N.err" | tail -1 > "$OUT/full_$N.json" &&
  timeout -k 10 300 python bench.py 2>>"$OUT/$N.err" | tail -1 > "$OUT/default_$N.json" &&
  (cd "$W" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$N" -o p -- \
      python "$ROOT/bench.py" --full --steps 10 --warmup 2 --cpu-seconds 0 --no-extras --no-split > "$OUT/prof_$N.json" 2>>"$OUT/$N.err") &&
  cp "$(find "$OUT/prof_$N" -name '*kernel_stats.csv' | head -1)" "$OUT/kernel_stats_$N.csv" && rm -rf "$OUT/prof_$N"
}
for i in $(seq 1 "$PAIRS"); do
  one tree "$TREE" "$i" && one variant "$VAR" "$i" || { echo "run $i failed: stopping (see $OUT/*.err)"; exit 1; }
done
python - "$OUT" "$PAIRS" "${AB_KERNEL:-k_idct_color<1>}" "${AB_STAGE:-idct_color}" <<'PY'
import csv, json, sys
out, pairs, kernel, stage = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
def row(name, i):
    f = json.load(open("%s/full_%s_%d.json" % (out, name, i))); d = json.load(open("%s/default_%s_%d.json" % (out, name, i)))
    k = [r for r in csv.reader(open("%s/kernel_stats_%s_%d.csv" % (out, name, i))) if kernel in r[0]][0]      # Name, Calls, TotalDurationNs, AverageNs, ...
    return dict(stage=f["roofline"]["stages_ms"][stage], one_stream=f["one_stream"]["ms_per_step"], step=d["ms_per_step"],
                exact=bool(f["bit_exact"]) and bool(d["bit_exact"]), kernel=float(k[3]) / 1e6)
rows = {(n, i): row(n, i) for n in ("tree", "variant") for i in range(1, pairs + 1)}
print("%-10s %10s %12s %12s %12s  %s" % ("run", stage, "one-stream", "ms_per_step", "kernel avg", "bit-exact"))
for i in range(1, pairs + 1):
    for n in ("tree", "variant"):
        r = rows[n, i]
        print("%-10s %10.3f %12.3f %12.3f %12.4f  %s" % ("%s %d" % (n, i), r["stage"], r["one_stream"], r["step"], r["kernel"], r["exact"]))
for key in ("stage", "one_stream", "step", "kernel"):
    t = [rows["tree", i][key] for i in range(1, pairs + 1)]; v = [rows["variant", i][key] for i in range(1, pairs + 1)]
    spread = max(max(t) - min(t), max(v) - min(v))
    gains = [v[i] - t[i] for i in range(pairs)]
    print("%-10s variant - tree per pair: %s; largest same-library spread %.4f; smallest gap between the two %.4f" %
          (key, " ".join("%+.4f" % g for g in gains), spread, min(v) - max(t)))
PY
