#!/bin/bash
# `ris -j` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one run each:
# plain vs -u vs -j, -t vs -t -u vs -t -j, default PRB_BATCH.  Prints lines, bytes and wall time of every run, checks that
# the -j lines are lines of the plain run, and gives - one batch of the same queries through the C ABI, with neither
# option, with distinct_sites and with chain_sites - the device time of the "distinct" and "chain" stages beside
# "filter" and "traceback".
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/chain_throughput.sh [N=64]
N=${1:-64}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000
# run NAME FLAGS...: ris with FLAGS under a time limit; its wall time and queries/s; the size of its output file
run() {
  local name=$1
  shift
  python3 -c 'import subprocess, sys, time
t = time.time()
rc = subprocess.call(["timeout", "-k", "10", "600"] + sys.argv[3:])
w = time.time() - t
print(f"{sys.argv[1]}: {w:.2f} s, {int(sys.argv[2]) / w:.2f} queries/s")
sys.exit(rc)' "$name" "$N" "$BIN" ris "$@" -i "$W/cs_q.fa" -o "$W/cs_$name.out" -d "$DB" &&
    echo "$name: $(stat -c %s "$W/cs_$name.out") bytes, $(($(wc -l < "$W/cs_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/cs_q.fa" &&
  run plain && run u -u && run j -j && run t -t && run tu -t -u && run tj -t -j &&
  timeout -k 10 600 python3 - "$W/cs_j.out" "$W/cs_plain.out" <<'EOF2' &&
import sys
kept = [l.split(",", 1)[1] for l in open(sys.argv[1]).read().splitlines()[3:]]
at, full = 0, 0
with open(sys.argv[2]) as f:  # (the full text is read line by line: it is gigabytes) - the -j lines, in order, among its lines
    for i, l in enumerate(f):
        if i < 3:
            continue
        full += 1
        if at < len(kept) and l.rstrip("\n").split(",", 1)[1] == kept[at]:
            at += 1
print(f"-j: {len(kept)} of the plain run's {full} lines, in its order: {at == len(kept)}")
sys.exit(0 if at == len(kept) else 1)
EOF2
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/cs_q.fa" "$DB" <<'EOF2'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
STAGES = ("distinct", "chain", "filter", "traceback", "traceback_slow")
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    for p in range(db.npages):  # warm-up (buffers grow to the batch)
        capi.search_page_summary(ctx, qb, db, p)
    for name, kw in (("neither", {}), ("distinct_sites=1", dict(distinct_sites=1)), ("chain_sites=1", dict(chain_sites=1))):
        opts = capi.default_opts(**kw)
        ctx.reset_timers()
        returned = final = 0
        for p in range(db.npages):
            pairs, counts = capi.search_page_summary(ctx, qb, db, p, opts, with_counts=True)
            returned, final = returned + int(pairs["hits"].sum()), final + counts[2]
        ms = {s: ctx.stage_ms(s) for s in STAGES}
        print(f"summary, {name}: {returned} of {final} final hits kept; device ms (launches): " +
              ", ".join(f"{s} {ms[s][0]:.2f} ({ms[s][1]})" for s in STAGES))
    qb.close()
    db.close()
EOF2
  ) && rm -f "$W"/cs_*.out
