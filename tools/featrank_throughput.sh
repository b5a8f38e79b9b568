#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, the annotation
# the three consecutive thirds of every target - the input of ftop_throughput.sh -: every query-feature line (-t -A)
# against the 20 best queries per feature (-t -A -B 20).  Each run once to warm the page cache, then RUNS times: prints
# the median wall time and the spread, the bytes and lines written and the peak resident set of the process, and gives the
# device time of the "feature" and "featrank" stages (one batch of the same queries through the C ABI, a warm-up pass
# first, then RUNS passes: median and spread) with the step time, and the ranking table's HBM footprint.  Every step runs
# under a time limit of its own; the first failure ends the script.
# usage: tools/featrank_throughput.sh [N=16] [RUNS=5]      (BIN=PATH SKIP_FEATRANK=1: the -t -A run alone, with another build's binary)
N=${1:-16}
RUNS=${2:-5}
K=20
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=${BIN:-$HERE/priblast_amd/bin/pRIblast-hip}
DB=$W/db_s50000x2000
# run NAME CMD...: CMD under a time limit, once unmeasured and RUNS times measured; its peak resident set and its output file
run() {
  local name=$1
  shift
  python3 -c 'import resource, statistics, subprocess, sys, time
runs, walls = int(sys.argv[2]), []
for k in range(runs + 1):
    t = time.time()
    rc = subprocess.call(["timeout", "-k", "10", "600"] + sys.argv[3:])
    if rc:
        sys.exit(rc)
    if k:
        walls.append(time.time() - t)
rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024
print(f"{sys.argv[1]}: median {statistics.median(walls):.2f} s of {runs} warm runs (min {min(walls):.2f}, max {max(walls):.2f}), peak RSS {rss:.0f} MB")' \
    "$name" "$RUNS" "$@" && echo "$name: $(stat -c %s "$W/frt_$name.out") bytes, $(($(wc -l < "$W/frt_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/frt_q.fa" &&
  (cd "$HERE" && timeout -k 10 300 python3 - "$DB" "$W/frt_features.tsv" <<'EOF2'
import sys
from priblast_amd import capi
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[1])
    rows = [(db.seq_name(p, i), db.seq_lengths(p, i)[0]) for p in range(db.npages) for i in range(db.page_info(p)[0])]
    db.close()
with open(sys.argv[2], "w") as f:
    f.writelines(f"{n}\t{k * l // 3}\t{(k + 1) * l // 3 - 1}\tthird{k}\n" for n, l in rows for k in range(3))
print(f"annotation file: {3 * len(rows)} features on {len(rows)} targets")
EOF2
  ) &&
  run feature "$BIN" ris -t -A "$W/frt_features.tsv" -i "$W/frt_q.fa" -o "$W/frt_feature.out" -d "$DB" &&
  { [ -n "$SKIP_FEATRANK" ] || run featrank "$BIN" ris -t -A "$W/frt_features.tsv" -B "$K" -i "$W/frt_q.fa" -o "$W/frt_featrank.out" -d "$DB"; } &&
  { [ -n "$SKIP_FEATRANK" ] || (cd "$HERE" && timeout -k 10 600 python3 - "$W/frt_q.fa" "$DB" "$K" "$RUNS" <<'EOF2'
import statistics
import sys
import time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k, runs = int(sys.argv[3]), int(sys.argv[4])
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
            annot += [(p, i, j * length // 3, (j + 1) * length // 3 - 1) for j in range(3)]
    ids = list(range(len(seqs)))
    rows = {"feature": [], "featrank": []}
    with capi.Annotation(ctx, db, annot) as an:
        for r in range(runs + 1):  # (the first pass warms up: buffers grow to the batch)
            for mode in rows:
                ctx.reset_timers()
                t0 = time.time()
                recs = capi.search_features(ctx, qb, db, an)[0] if mode == "feature" else capi.search_featrank(ctx, db, an, k, [(qb, ids)])[0]
                wall = (time.time() - t0) * 1e3
                if r:
                    rows[mode].append((wall, sum(ctx.stage_ms(s)[0] for s in SEARCH), ctx.stage_ms("summary")[0], ctx.stage_ms("feature")[0],
                                       ctx.stage_ms("feature")[1], ctx.stage_ms("featrank")[0], ctx.stage_ms("featrank")[1], len(recs)))
    for mode, v in rows.items():
        med = lambda c: statistics.median(x[c] for x in v)
        spread = lambda c: f"{min(x[c] for x in v):.2f}-{max(x[c] for x in v):.2f}"
        print(f"{mode}: step {med(0):.1f} ms ({spread(0)}), search stages {med(1):.1f} ms, summary {med(2):.2f} ms, "
              f"feature stage {med(3):.2f} ms ({spread(3)}; {v[0][4]} launches), featrank stage {med(5):.2f} ms ({spread(5)}; {v[0][6]} launches), "
              f"{v[0][7]} records; medians of {runs} warm passes, {len(seqs)} queries, {len(annot)} features")
    table = len(annot) * k * (16 + capi.FEATRANK_DTYPE.itemsize) + (len(annot) + 1) * 4
    print(f"feature ranking table: {table / 2 ** 20:.1f} MB of HBM for {len(annot)} features of {k} slots")
    qb.close()
    db.close()
EOF2
  ); } && rm -f "$W/frt_feature.out" "$W/frt_featrank.out"
