#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, three
# times: the full result lines, the 20 best pairs per query (-t -n 20), the 20 best interaction sites per query (-k 20),
# default PRB_BATCH.  Prints wall time, queries/s, peak RSS, output bytes and lines of each run, checks the -k lines
# against the full ones, and gives the device time of the "tophits" stage (prb_search_page_tophits, one batch of the same
# queries through the C ABI) beside that of the "top" stage.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/tophits_throughput.sh [N=64]
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
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/th_$name.out") bytes, $(($(wc -l < "$W/th_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/th_q.fa" &&
  run full "$BIN" ris -i "$W/th_q.fa" -o "$W/th_full.out" -d "$DB" &&
  run top "$BIN" ris -t -n "$K" -i "$W/th_q.fa" -o "$W/th_top.out" -d "$DB" &&
  run tophits "$BIN" ris -k "$K" -i "$W/th_q.fa" -o "$W/th_tophits.out" -d "$DB" &&
  timeout -k 10 600 python3 - "$W/th_tophits.out" "$W/th_full.out" "$N" "$K" <<'EOF2' &&
import sys
n, k = int(sys.argv[3]), int(sys.argv[4])
kept = [l.split(",", 1)[1] for l in open(sys.argv[1]).read().splitlines()[3:]]
energy = lambda l: float(l.split(",")[6])  # Interaction Energy, as printed (the Id is stripped)
by_q, lowest, lines = {}, {}, {}
for l in kept:
    by_q.setdefault(l.split(",", 1)[0], []).append(l)
want = set(kept)
with open(sys.argv[2]) as f:  # (the full text is read line by line: it is gigabytes)
    for i, l in enumerate(f):
        if i < 3:
            continue
        l = l.rstrip("\n").split(",", 1)[1]
        want.discard(l)
        v = lowest.setdefault(l.split(",", 1)[0], [])
        v.append(energy(l))
        if len(v) > 65536:  # (hundreds of thousands of lines per query: only the k lowest are kept)
            v[:] = sorted(v)[:k]
# per query: the lines are full lines, ascending in energy, and their energies are the k lowest of the query's lines
# (compared as printed: two energies that print alike may come in either order)
best = not want and all([energy(l) for l in v] == sorted(lowest[q])[:k] for q, v in by_q.items())
print(f"tophits: {len(kept)} lines for {len(by_q)} queries (expected {n} x {k} = {n * k}); every query's lines are the {k} "
      f"lowest-energy result lines of that query, best first: {best}")
sys.exit(0 if best and len(kept) == n * k else 1)
EOF2
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/th_q.fa" "$DB" "$K" <<'EOF2'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k = int(sys.argv[3])
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_tophits(ctx, qb, db, k)  # warm-up (buffers grow to the batch)
    ctx.reset_timers()
    recs, bp = capi.search_tophits(ctx, qb, db, k)
    t, tl = ctx.stage_ms("tophits")
    step = sum(ctx.stage_ms(s)[0] for s in ("seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2",
                                            "gapped_t3", "gapped_slow", "traceback", "traceback_slow", "tophits"))
    print(f"tophits stage: {t:.2f} ms for {len(seqs)} queries ({tl} launches, {len(recs)} records and {len(bp)} pairs kept), "
          f"{100 * t / step:.2f} % of the {step:.0f} ms of device time of the search stages")
    ctx.reset_timers()
    capi.search_top(ctx, qb, db, k)
    t, tl = ctx.stage_ms("top")
    s, sl = ctx.stage_ms("summary")
    print(f"top stage, same batch: {t:.2f} ms ({tl} launches); summary stage before it: {s:.2f} ms ({sl} launches)")
    qb.close()
    db.close()
EOF2
  ) && rm -f "$W/th_full.out" "$W/th_top.out" "$W/th_tophits.out"
