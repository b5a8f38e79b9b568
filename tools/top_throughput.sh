#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, twice:
# per-pair summary lines (-t), then the 20 best pairs per query (-t -n 20), default PRB_BATCH.  Prints wall time,
# queries/s, peak RSS, output bytes and lines of each run, and the device time of the "top" stage (prb_search_page_top,
# one batch of the same queries through the C ABI) beside the "summary" stage it follows.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/top_throughput.sh [N=64]
N=${1:-64}
K=20
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
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/tt_$name.out") bytes, $(($(wc -l < "$W/tt_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/tt_q.fa" &&
  run summary "$BIN" ris -t -i "$W/tt_q.fa" -o "$W/tt_summary.out" -d "$DB" &&
  run top "$BIN" ris -t -n "$K" -i "$W/tt_q.fa" -o "$W/tt_top.out" -d "$DB" &&
  timeout -k 10 300 python3 - "$W/tt_top.out" "$W/tt_summary.out" "$N" "$K" <<'EOF' &&
import sys
top = [l.split(",", 1)[1] for l in open(sys.argv[1]).read().splitlines()[3:]]
full = [l.split(",", 1)[1] for l in open(sys.argv[2]).read().splitlines()[3:]]
n, k = int(sys.argv[3]), int(sys.argv[4])
def by_query(lines):
    d = {}
    for l in lines:
        d.setdefault(l.split(",", 1)[0], []).append(l)
    return d
energy = lambda l: float(l.split(",")[5])  # Minimum Interaction Energy, as printed
tq, fq = by_query(top), by_query(full)
# per query: the lines are -t lines, ascending in energy, and their energies are the k lowest of the query's -t lines
# (compared as printed: two energies that print alike may come in either order)
best = all(set(v) <= set(fq[q]) and [energy(l) for l in v] == sorted(energy(l) for l in fq[q])[:k] for q, v in tq.items())
print(f"top: {len(top)} lines for {len(tq)} queries (expected {n} x {k} = {n * k}); every query's lines are the {k} "
      f"lowest-energy -t lines of that query, best first: {best}")
sys.exit(0 if best and len(top) == n * k else 1)
EOF
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/tt_q.fa" "$DB" "$K" <<'EOF'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k = int(sys.argv[3])
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_top(ctx, qb, db, k)  # warm-up (buffers grow to the batch)
    ctx.reset_timers()
    n = len(capi.search_top(ctx, qb, db, k))
    t, tl = ctx.stage_ms("top")
    s, sl = ctx.stage_ms("summary")
    print(f"top stage: {t:.2f} ms for {len(seqs)} queries ({tl} launches, {n} records kept); "
          f"summary stage before it: {s:.2f} ms ({sl} launches)")
    qb.close()
    db.close()
EOF
  ) && rm -f "$W/tt_summary.out" "$W/tt_top.out"
