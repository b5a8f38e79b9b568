#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries: one line per
# pair (-t) against one line per query-feature pair (-t -A), the annotation giving every target three features: the first
# 10 %, the middle 60 % and the last 30 % of its length.  Each run once to warm the page cache, then RUNS times: prints
# the median wall time and the spread, output bytes and lines, and gives the device time of the "summary" and "feature"
# stages with their launches, the records and the unassigned hits (one batch of the same queries through the C ABI, a
# warm-up pass first, then RUNS passes: median and spread).  PARENT_BIN: another build's pRIblast-hip, whose -t is timed
# the same way on the same input (the parent commit's, to tell what this build's -t costs beside it).
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/feature_throughput.sh [N=16] [RUNS=3]
N=${1:-16}
RUNS=${2:-3}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000
# run NAME CMD...: CMD under a time limit, once unmeasured and RUNS times measured; the size of its output file
run() {
  local name=$1
  shift
  python3 -c 'import statistics, subprocess, sys, time
runs, walls = int(sys.argv[2]), []
for k in range(runs + 1):
    t = time.time()
    rc = subprocess.call(["timeout", "-k", "10", "600"] + sys.argv[3:])
    if rc:
        sys.exit(rc)
    if k:
        walls.append(time.time() - t)
print(f"{sys.argv[1]}: median {statistics.median(walls):.2f} s of {runs} warm runs (min {min(walls):.2f}, max {max(walls):.2f}; " +
      ", ".join(f"{w:.2f}" for w in walls) + ")")' \
    "$name" "$RUNS" "$@" && echo "$name: $(stat -c %s "$W/ft_$name.out") bytes, $(($(wc -l < "$W/ft_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/ft_q.fa" &&
  (cd "$HERE" && timeout -k 10 300 python3 - "$DB" "$W/ft_features.tsv" <<'EOF2'
import sys
from priblast_amd import capi
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[1])
    seqs = [(db.seq_name(p, i), db.seq_lengths(p, i)[0]) for p in range(db.npages) for i in range(db.page_info(p)[0])]
    db.close()
with open(sys.argv[2], "w") as f:
    for n, length in seqs:
        a, b = length // 10, length - 3 * length // 10
        f.write(f"{n}\t0\t{a - 1}\thead\n{n}\t{a}\t{b - 1}\tbody\n{n}\t{b}\t{length - 1}\ttail\n")
print(f"annotation file: {len(seqs)} targets, {3 * len(seqs)} features")
EOF2
  ) &&
  { [ -z "$PARENT_BIN" ] || run parent_pairs "$PARENT_BIN" ris -t -i "$W/ft_q.fa" -o "$W/ft_parent_pairs.out" -d "$DB"; } &&
  run pairs "$BIN" ris -t -i "$W/ft_q.fa" -o "$W/ft_pairs.out" -d "$DB" &&
  run features "$BIN" ris -t -A "$W/ft_features.tsv" -i "$W/ft_q.fa" -o "$W/ft_features.out" -d "$DB" &&
  { [ -z "$PARENT_BIN" ] || { cmp "$W/ft_parent_pairs.out" "$W/ft_pairs.out" && echo "pairs: the same bytes as parent_pairs"; }; } &&
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/ft_q.fa" "$DB" "$RUNS" <<'EOF2'
import statistics
import sys
import time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
runs = int(sys.argv[3])
SEARCH = ("seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow", "traceback",
          "traceback_slow")
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    annot = []
    for p in range(db.npages):
        for i in range(db.page_info(p)[0]):
            length = db.seq_lengths(p, i)[0]
            a, b = length // 10, length - 3 * length // 10
            annot += [(p, i, 0, a - 1), (p, i, a, b - 1), (p, i, b, length - 1)]
    rows = {"pairs": [], "features": []}
    with capi.Annotation(ctx, db, annot) as an:
        for r in range(runs + 1):  # (the first pass warms up: buffers grow to the batch)
            for mode in ("pairs", "features"):
                ctx.reset_timers()
                t0 = time.time()
                if mode == "pairs":
                    n, un = sum(len(capi.search_page_summary(ctx, qb, db, p)) for p in range(db.npages)), 0
                else:
                    recs, un = capi.search_features(ctx, qb, db, an)
                    n = len(recs)
                wall = (time.time() - t0) * 1e3
                if r:
                    rows[mode].append((wall, sum(ctx.stage_ms(s)[0] for s in SEARCH), ctx.stage_ms("summary")[0], ctx.stage_ms("summary")[1],
                                       ctx.stage_ms("feature")[0], ctx.stage_ms("feature")[1], n, un))
    for mode, v in rows.items():
        med = lambda c: statistics.median(x[c] for x in v)
        spread = lambda c: f"{min(x[c] for x in v):.2f}-{max(x[c] for x in v):.2f}"
        print(f"{mode}: step {med(0):.1f} ms ({spread(0)}), search stages {med(1):.1f} ms, summary {med(2):.2f} ms ({spread(2)}; {v[0][3]} launches), "
              f"feature stage {med(4):.2f} ms ({spread(4)}; {v[0][5]} launches), {v[0][6]} records, {v[0][7]} unassigned hits; medians of {runs} "
              f"warm passes, {len(seqs)} queries, {len(annot)} features")
    qb.close()
    db.close()
EOF2
  ) && rm -f "$W/ft_pairs.out" "$W/ft_features.out" "$W/ft_parent_pairs.out"
