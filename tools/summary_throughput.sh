#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, twice:
# full result lines, then per-pair summary lines (-t).  Prints queries/s, output bytes and the peak RSS of each run, the
# skew of the pairs' hit counts, and the device time of the "summary" stage (prb_search_page_summary, one batch of the
# same queries through the C ABI) beside the base-pair stage it follows.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/summary_throughput.sh [N=16]
N=${1:-16}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000
# run NAME CMD...: CMD under a time limit; its wall time, queries/s and peak RSS; the size of its output file
run() {
  local name=$1
  shift
  python3 -c 'import resource, subprocess, sys, time
t = time.time()
rc = subprocess.call(["timeout", "-k", "10", "600"] + sys.argv[3:])
w = time.time() - t
rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024
print(f"{sys.argv[1]}: {w:.2f} s, {int(sys.argv[2]) / w:.2f} queries/s, peak RSS {rss:.0f} MB")
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/st_$name.out") bytes, $(($(wc -l < "$W/st_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/st_q.fa" &&
  run full "$BIN" ris -i "$W/st_q.fa" -o "$W/st_full.out" -d "$DB" &&
  run summary "$BIN" ris -t -i "$W/st_q.fa" -o "$W/st_summary.out" -d "$DB" &&
  python3 - "$W/st_summary.out" "$W/st_full.out" <<'EOF' &&
import sys
hits = [int(l.split(",")[5]) for l in open(sys.argv[1]).read().splitlines()[3:]]
full = sum(1 for _ in open(sys.argv[2])) - 3
hits.sort()
print(f"pairs {len(hits)}, hits in them {sum(hits)} (full output: {full} lines), hits per pair: mean {sum(hits) / len(hits):.1f}, "
      f"median {hits[len(hits) // 2]}, p99 {hits[int(len(hits) * 0.99)]}, p99.99 {hits[int(len(hits) * 0.9999)]}, max {hits[-1]}")
EOF
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/st_q.fa" "$DB" <<'EOF'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    for p in range(db.npages):  # warm-up (buffers grow to the batch)
        capi.search_page_summary(ctx, qb, db, p)
    ctx.reset_timers()
    n = sum(len(capi.search_page_summary(ctx, qb, db, p)) for p in range(db.npages))
    s, l = ctx.stage_ms("summary")
    t, _ = ctx.stage_ms("traceback")
    print(f"summary stage: {s:.2f} ms for {len(seqs)} queries ({l} launches, {n} pairs); base pairs before it: {t:.2f} ms")
    qb.close()
    db.close()
EOF
  ) && rm -f "$W/st_full.out"
