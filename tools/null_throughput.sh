#!/bin/bash
# `ris -t -z 10` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one batch
# through the C ABI: the per-pair summaries alone (`-t`) against the null table with 10 decoys per query, its decoy
# batches searched under the mask of their owners' observed targets (the default) and without it (PRB_NULL_MASK=0).  Per
# run the wall time, the stage counts of the real batch and of the decoys, the observed pairs, and the device time of the
# stages "null" (the scatter, the fold and the finish), "allow" (the mask's test and compaction) and "seed", with the
# sum of the stages behind the seeds.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/null_throughput.sh [N=4] [DECOYS=10]
N=${1:-4}
Z=${2:-10}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/null_q.fa" "$DB" "$Z" <<'EOF2'
import sys, time
import numpy as np
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys = int(sys.argv[3])
STAGES = ("null", "allow", "seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow",
          "traceback", "traceback_slow", "summary", "raccess")
BEHIND = STAGES[3:14]  # what lies behind the seed stage
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_page_summary(ctx, qb, db, 0)  # warm-up (buffers grow to the batch)

    def report(name, wall, extra):
        ms = {s: ctx.stage_ms(s)[0] for s in STAGES}
        print(f"{name}: wall {wall:.3f} s; {extra}; null {ms['null']:.2f} ms ({ctx.stage_ms('null')[1]} launches), allow {ms['allow']:.1f} ms, "
              f"seed {ms['seed']:.1f} ms, behind the seed stage {sum(ms[s] for s in BEHIND):.1f} ms, raccess {ms['raccess']:.1f} ms")

    ctx.reset_timers()
    t0 = time.time()
    got = [capi.search_page_summary(ctx, qb, db, p, with_counts=True) for p in range(db.npages)]
    report("-t", time.time() - t0, f"pairs {sum(len(r) for r, _ in got)}, seeds / ungapped / final {np.sum([c for _, c in got], 0).tolist()}")
    tables = {}
    for mask in (True, False):
        ctx.reset_timers()
        t0 = time.time()
        recs, counts, dcounts = capi.search_null(ctx, qb, seqs, db, ndecoys, mask=mask, with_counts=True)
        tables[mask] = recs
        report(f"-t -z {ndecoys}" + ("" if mask else " PRB_NULL_MASK=0"), time.time() - t0,
               f"pairs {len(recs)}, real {list(counts)}, decoys {list(dcounts)}, NullHits {int(recs['null_hits'].sum())}, "
               f"NullLE {int(recs['null_le'].sum())}, pairs with p <= {1.0 / (ndecoys + 1):.3f}: {int((recs['null_le'] == 0).sum())}")
    assert tables[True].tobytes() == tables[False].tobytes(), "the mask changed the table"
    print("the two tables are the same bytes")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/null_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each" && table
