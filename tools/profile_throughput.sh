#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, twice:
# per-pair summary lines (-t), then the per-position profile (-q), default PRB_BATCH.  Prints wall time, queries/s,
# peak RSS, output bytes and lines of each run, checks the profile lines' shape, and prints the device time of the
# "profile" stage (prb_search_page_profile + prb_profset_finish, one batch of the same queries through the C ABI) beside
# the "summary" stage (pair runs) in front of it.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/profile_throughput.sh [N=64]
N=${1:-64}
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
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/pt_$name.out") bytes, $(($(wc -l < "$W/pt_$name.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/pt_q.fa" &&
  run summary "$BIN" ris -t -i "$W/pt_q.fa" -o "$W/pt_summary.out" -d "$DB" &&
  run profile "$BIN" ris -q -i "$W/pt_q.fa" -o "$W/pt_profile.out" -d "$DB" &&
  timeout -k 10 300 python3 - "$W/pt_profile.out" "$W/pt_summary.out" "$N" <<'PY' &&
import sys
prof = [l.split(",") for l in open(sys.argv[1]).read().splitlines()[3:]]
pairs = {}
for l in open(sys.argv[2]).read().splitlines()[3:]:
    q = l.split(",", 2)[1]
    pairs[q] = pairs.get(q, 0) + 1
n = int(sys.argv[3])
# consecutive Ids; positions ascending within a query; 1 <= Targets <= Hits; Targets at most the query's -t lines (its
# pairs); the queries those of the -t output
ok = [int(f[0]) for f in prof] == list(range(len(prof)))
last = {}
for f in prof:
    q, pos, hits, tg = f[1], int(f[3]), int(f[4]), int(f[5])
    ok = ok and pos > last.get(q, -1) and 1 <= tg <= hits and tg <= pairs.get(q, 0)
    last[q] = pos
ok = ok and set(last) == set(pairs)
print(f"profile: {len(prof)} lines for {len(last)} queries ({n} x 2 kb: at most {n * 2000}); Ids, position order, "
      f"1 <= Targets <= Hits and Targets <= the query's -t lines: {ok}")
sys.exit(0 if ok and len(prof) <= n * 2000 else 1)
PY
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/pt_q.fa" "$DB" <<'PY'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_profile(ctx, qb, db)  # warm-up (buffers grow to the batch)
    ctx.reset_timers()
    n = len(capi.search_profile(ctx, qb, db))
    t, tl = ctx.stage_ms("profile")
    s, sl = ctx.stage_ms("summary")
    print(f"profile stage: {t:.2f} ms for {len(seqs)} queries ({tl} launches, {n} rows); "
          f"summary stage before it: {s:.2f} ms ({sl} launches)")
    qb.close()
    db.close()
PY
  ) && rm -f "$W/pt_summary.out" "$W/pt_profile.out"
