#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, three
# times: per-pair summary lines (-t), then the targets' regions at depth 1 and at depth 4 (-c 1, -c 4), default
# PRB_BATCH.  Prints wall time, queries/s, peak RSS, output bytes and lines of each run, checks the region lines' shape
# against the -t lines, and prints the device time of the "coverage" stage per sub-batch merge and per finish (one batch
# of the same queries through the C ABI).
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/coverage_throughput.sh [N=16]
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
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/ct_$name.out") bytes, $(($(wc -l < "$W/ct_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/ct_q.fa" &&
  run summary "$BIN" ris -t -i "$W/ct_q.fa" -o "$W/ct_summary.out" -d "$DB" &&
  run depth1 "$BIN" ris -c 1 -i "$W/ct_q.fa" -o "$W/ct_depth1.out" -d "$DB" &&
  run depth4 "$BIN" ris -c 4 -i "$W/ct_q.fa" -o "$W/ct_depth4.out" -d "$DB" &&
  timeout -k 10 300 python3 - "$W/ct_depth1.out" "$W/ct_depth4.out" "$W/ct_summary.out" <<'PY' &&
import sys
d1, d4 = ([l.split(",") for l in open(p).read().splitlines()[3:]] for p in sys.argv[1:3])
hits = {}
for l in open(sys.argv[3]).read().splitlines()[3:]:
    f = l.split(",")
    hits[f[3]] = hits.get(f[3], 0) + int(f[5])
# consecutive Ids; Start <= End <= Target Length - 1; a target's regions apart and ascending; depth 1: every target of
# the -t lines, its regions' Hits summing to its -t hit counts; depth 4: Max Queries >= 4, inside a region of depth 1
ok = all([int(f[0]) for f in d] == list(range(len(d))) for d in (d1, d4))
got, spans, last = {}, {}, (None, -2)
for d in (d1, d4):
    for f in d:
        name, length, start, end = f[1], int(f[2]), int(f[3]), int(f[4])
        ok = ok and 0 <= start <= end < length and int(f[7]) >= (1 if d is d1 else 4) and start <= int(f[8]) <= end
        ok = ok and (name != last[0] or start > last[1] + 1)
        last = (name, end)
        if d is d1:
            got[name] = got.get(name, 0) + int(f[5])
            spans.setdefault(name, []).append((start, end))
        else:
            ok = ok and any(a <= start and end <= b for a, b in spans.get(name, []))
    last = (None, -2)
ok = ok and got == hits
print(f"coverage: {len(d1)} regions of depth 1 on {len(got)} targets, {len(d4)} of depth 4; Ids, bounds, order, "
      f"depth 4 within depth 1 and Hits summed per target == the -t lines' hits: {ok}")
sys.exit(0 if ok else 1)
PY
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/ct_q.fa" "$DB" <<'PY'
import sys
import numpy as np
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ids = np.arange(len(seqs), dtype=np.int32)
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_coverage(ctx, db, 1, [(qb, ids)])  # warm-up (buffers grow to the batch)
    with capi.CovSet(ctx, db) as cs:
        ctx.reset_timers()
        for p in range(db.npages):
            cs.merge(qb, p, ids)
        m, ml = ctx.stage_ms("coverage")
        ctx.reset_timers()
        n = len(cs.finish(4))
        f, fl = ctx.stage_ms("coverage")
    print(f"coverage stage: merges {m:.2f} ms for {len(seqs)} queries ({ml} launches = {ml // 9} sub-batches: "
          f"{m / max(ml // 9, 1):.2f} ms each); finish at depth 4 {f:.2f} ms ({fl} launches, {n} regions)")
    qb.close()
    db.close()
PY
  ) && rm -f "$W/ct_summary.out" "$W/ct_depth1.out" "$W/ct_depth4.out"
