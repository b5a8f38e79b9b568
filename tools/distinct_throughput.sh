#!/bin/bash
# `ris -u` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one run each:
# plain vs -u, -k 20 vs -k 20 -u, -t vs -t -u, default PRB_BATCH.  Prints lines, bytes, wall time and peak RSS of every
# run, checks that the -u lines are lines of the plain run, and gives - one batch of the same queries through the C ABI,
# with and without the option - the device time of the "distinct", "filter", "traceback" and "tophits" stages.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/distinct_throughput.sh [N=64]
N=${1:-64}
K=20
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000
# run NAME FLAGS...: ris with FLAGS under a time limit; its wall time, queries/s and peak RSS; the size of its output file
run() {
  local name=$1
  shift
  python3 -c 'import resource, subprocess, sys, time
t = time.time()
rc = subprocess.call(["timeout", "-k", "10", "600"] + sys.argv[3:])
w = time.time() - t
rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024
print(f"{sys.argv[1]}: {w:.2f} s, {int(sys.argv[2]) / w:.2f} queries/s, peak RSS {rss:.0f} MB")
sys.exit(rc)' "$name" "$N" "$BIN" ris "$@" -i "$W/ds_q.fa" -o "$W/ds_$name.out" -d "$DB" &&
    echo "$name: $(stat -c %s "$W/ds_$name.out") bytes, $(($(wc -l < "$W/ds_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/ds_q.fa" &&
  run plain && run u -u && run k -k "$K" && run ku -k "$K" -u && run t -t && run tu -t -u &&
  timeout -k 10 600 python3 - "$W/ds_u.out" "$W/ds_plain.out" <<'EOF2' &&
import sys
kept = [l.split(",", 1)[1] for l in open(sys.argv[1]).read().splitlines()[3:]]
at, full = 0, 0
with open(sys.argv[2]) as f:  # (the full text is read line by line: it is gigabytes) - the -u lines, in order, among its lines
    for i, l in enumerate(f):
        if i < 3:
            continue
        full += 1
        if at < len(kept) and l.rstrip("\n").split(",", 1)[1] == kept[at]:
            at += 1
print(f"-u: {len(kept)} of the plain run's {full} lines, in its order: {at == len(kept)}")
sys.exit(0 if at == len(kept) else 1)
EOF2
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/ds_q.fa" "$DB" "$K" <<'EOF2'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k = int(sys.argv[3])
STAGES = ("distinct", "filter", "traceback", "traceback_slow", "tophits")
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_tophits(ctx, qb, db, k)  # warm-up (buffers grow to the batch)
    for u in (0, 1):
        opts = capi.default_opts(distinct_sites=u)
        ctx.reset_timers()
        returned = final = 0
        for p in range(db.npages):
            hits, bp, counts = capi.search_page(ctx, qb, db, p, opts)
            returned, final = returned + len(hits), final + counts[2]
            del hits, bp
        ms = {s: ctx.stage_ms(s) for s in STAGES}
        print(f"hits, distinct_sites={u}: {returned} of {final} final hits returned; device ms (launches): " +
              ", ".join(f"{s} {ms[s][0]:.2f} ({ms[s][1]})" for s in STAGES))
        ctx.reset_timers()
        recs, _ = capi.search_tophits(ctx, qb, db, k, opts)
        ms = {s: ctx.stage_ms(s) for s in STAGES}
        print(f"tophits {k}, distinct_sites={u}: {len(recs)} records; device ms (launches): " +
              ", ".join(f"{s} {ms[s][0]:.2f} ({ms[s][1]})" for s in STAGES))
    qb.close()
    db.close()
EOF2
  ) && rm -f "$W"/ds_*.out
