#!/bin/bash
# The command line for ONE 2 kb query against bench.py's configs[2] database rebuilt with `db -c` into 8 pages (cached
# beside bench.py's copy, built if missing): one worker (PRB_DEVICES=0) against two workers that share the pages of the
# one batch (PRB_DEVICES=0,0 PRB_SPLIT=pages), for the full result lines, -t -n 20, -k 20 and -q, REPS times each.  Prints
# wall time and peak RSS of each run and the split's own report, checks that the two settings write the same bytes, and
# gives the device time of the table merges (prb_*_merge, 64 queries through the C ABI: pages 0-3 and 4-7 in two tables)
# beside the "top" / "tophits" / "profile" stage times of the searches that filled them.
# With both workers on one GPU no speed-up is to be expected: the rows show what the split costs there.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/split_throughput.sh [REPS=3]
REPS=${1:-3}
K=20
PAGES=8
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000_c$PAGES
mkdir -p "$W" || exit 1
# run NAME ENV... -- CMD...: CMD under a time limit with ENV set; its wall time and peak RSS, and the split's report
run() {
  local name=$1
  shift
  python3 -c 'import os, resource, subprocess, sys, time
cut = sys.argv.index("--")
env = dict(os.environ, **dict(kv.split("=", 1) for kv in sys.argv[2:cut]))
t = time.time()
p = subprocess.run(["timeout", "-k", "10", "300"] + sys.argv[cut + 1:], env=env, stderr=subprocess.PIPE, text=True)
w = time.time() - t
rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024
note = "".join("; " + l for l in p.stderr.splitlines() if l.startswith("page split"))
sys.stderr.write("".join(l + "\n" for l in p.stderr.splitlines() if not l.startswith("page split")))
print(f"{sys.argv[1]}: {w:.2f} s, peak RSS {rss:.0f} MB{note}")
sys.exit(p.returncode)' "$name" "$@"
}
# row NAME SWITCHES...: REPS runs of either setting, then the comparison of what they wrote
row() {
  local name=$1 i
  shift
  for i in $(seq "$REPS"); do
    run "$name one worker #$i" PRB_DEVICES=0 -- "$BIN" ris "$@" -i "$W/sp_q.fa" -o "$W/sp_one.out" -d "$DB" || return 1
  done
  for i in $(seq "$REPS"); do
    run "$name two workers, pages split #$i" PRB_DEVICES=0,0 PRB_SPLIT=pages -- "$BIN" ris "$@" -i "$W/sp_q.fa" -o "$W/sp_two.out" -d "$DB" || return 1
  done
  cmp "$W/sp_one.out" "$W/sp_two.out" && echo "$name: same bytes ($(stat -c %s "$W/sp_one.out") bytes, $(($(wc -l < "$W/sp_one.out") - 3)) lines)"
}
if [ ! -e "$DB.stamp" ]; then
  (cd "$HERE" && timeout -k 10 900 python3 - "$DB" "$PAGES" <<'EOF2'
import sys, time
sys.path.insert(0, "tools")
import gen_synthetic
from priblast_amd import capi
prefix, pages = sys.argv[1], int(sys.argv[2])
recs = gen_synthetic.gen_fixed(50000, 2000, 1, "db")  # bench.py's configs[2] sequences
t = time.time()
with capi.Context(0) as ctx:
    capi.db_build(ctx, prefix, [r[0] for r in recs], [r[1] for r in recs], 0, 8, 70, 5, page_size=(len(recs) + pages - 1) // pages)
open(prefix + ".stamp", "w").write("built\n")
print(f"database of {pages} pages built in {time.time() - t:.1f} s")
EOF2
  ) || exit 1
fi
timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n 1 -L 2000 --seed 2 --prefix q -o "$W/sp_q.fa" &&
  row full &&
  row top -t -n "$K" &&
  row tophits -k "$K" &&
  row profile -q &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n 64 -L 2000 --seed 2 --prefix q -o "$W/sp_q64.fa" &&
  (cd "$HERE" && timeout -k 10 600 python3 - "$W/sp_q64.fa" "$DB" "$K" <<'EOF2'
import sys
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k = int(sys.argv[3])
with capi.Context(0) as a, capi.Context(0) as b:
    dbs = [capi.Db(a, sys.argv[2]), capi.Db(b, sys.argv[2])]
    qbs = []
    for ctx, db in zip((a, b), dbs):
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        qbs.append(qb)
    half = dbs[0].npages // 2
    for stage, make in (("top", lambda c, q: capi.TopSet(c, q, k)), ("tophits", lambda c, q: capi.TopHits(c, q, k)),
                        ("profile", lambda c, q: capi.ProfSet(c, q))):
        for timed in (False, True):  # (the first pass warms up: buffers grow to the batch)
            a.reset_timers()
            b.reset_timers()
            ta, tb = make(a, qbs[0]), make(b, qbs[1])
            for p in range(dbs[0].npages):
                (ta if p < half else tb).merge(dbs[0 if p < half else 1], p)
            filled = a.stage_ms(stage)[0] + b.stage_ms(stage)[0]
            a.reset_timers()
            ta.absorb(tb)
            ms, launches = a.stage_ms(stage)
            ta.close()
            tb.close()
        print(f"{stage}: merge of two tables {ms:.3f} ms ({launches} launches) for {len(seqs)} queries; the searches' own "
              f"\"{stage}\" stage over the {dbs[0].npages} pages: {filled:.2f} ms")
    for x in qbs + dbs:
        x.close()
EOF2
  ) && rm -f "$W/sp_one.out" "$W/sp_two.out"
