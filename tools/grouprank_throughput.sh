#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries: the 20 best
# groups per query (-t -G -n 20) against the 20 best queries per group (-t -G -R 20), the group file putting five
# consecutive targets into each group.  Each run once to warm the page cache, then RUNS times: prints the median wall time
# and the spread, the bytes and lines written and the peak resident set of the process, and gives the device time of the
# "group" and "grouprank" stages (one batch of the same queries through the C ABI, a warm-up pass first, then RUNS passes:
# median and spread) with the step time.  Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/grouprank_throughput.sh [N=16] [RUNS=5]
N=${1:-16}
RUNS=${2:-5}
K=20
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
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
    "$name" "$RUNS" "$@" && echo "$name: $(stat -c %s "$W/grt_$name.out") bytes, $(($(wc -l < "$W/grt_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/grt_q.fa" &&
  (cd "$HERE" && timeout -k 10 300 python3 - "$DB" "$W/grt_genes.tsv" <<'EOF2'
import sys
from priblast_amd import capi
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[1])
    names = [db.seq_name(p, i) for p in range(db.npages) for i in range(db.page_info(p)[0])]
    db.close()
with open(sys.argv[2], "w") as f:
    f.writelines(f"{n}\tgene{i // 5}\n" for i, n in enumerate(names))
print(f"group file: {len(names)} targets in {(len(names) + 4) // 5} groups")
EOF2
  ) &&
  run group "$BIN" ris -t -n "$K" -G "$W/grt_genes.tsv" -i "$W/grt_q.fa" -o "$W/grt_group.out" -d "$DB" &&
  run grouprank "$BIN" ris -t -R "$K" -G "$W/grt_genes.tsv" -i "$W/grt_q.fa" -o "$W/grt_grouprank.out" -d "$DB" &&
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/grt_q.fa" "$DB" "$K" "$RUNS" <<'EOF2'
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
    maps, t = [], 0
    for p in range(db.npages):
        nseq = db.page_info(p)[0]
        maps.append([(t + i) // 5 for i in range(nseq)])
        t += nseq
    ng = (t + 4) // 5
    ids = list(range(len(seqs)))
    rows = {"group": [], "grouprank": []}
    for r in range(runs + 1):  # (the first pass warms up: buffers grow to the batch)
        for mode in rows:
            ctx.reset_timers()
            t0 = time.time()
            recs = capi.search_groups(ctx, qb, db, maps, ng, k) if mode == "group" else capi.search_grouprank(ctx, db, maps, ng, k, [(qb, ids)])
            wall = (time.time() - t0) * 1e3
            if r:
                rows[mode].append((wall, sum(ctx.stage_ms(s)[0] for s in SEARCH), ctx.stage_ms("summary")[0], ctx.stage_ms("group")[0],
                                   ctx.stage_ms("group")[1], ctx.stage_ms("grouprank")[0], ctx.stage_ms("grouprank")[1], len(recs)))
    for mode, v in rows.items():
        med = lambda c: statistics.median(x[c] for x in v)
        spread = lambda c: f"{min(x[c] for x in v):.2f}-{max(x[c] for x in v):.2f}"
        print(f"{mode}: step {med(0):.1f} ms ({spread(0)}), search stages {med(1):.1f} ms, summary {med(2):.2f} ms, "
              f"group stage {med(3):.2f} ms ({spread(3)}; {v[0][4]} launches), grouprank stage {med(5):.2f} ms ({spread(5)}; {v[0][6]} launches), "
              f"{v[0][7]} records; medians of {runs} warm passes, {len(seqs)} queries, {ng} groups")
    qb.close()
    db.close()
EOF2
  ) && rm -f "$W/grt_group.out" "$W/grt_grouprank.out"
