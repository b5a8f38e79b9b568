#!/bin/bash
# `ris -t -A FILE -F 10` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one batch
# through the C ABI, the annotation the three consecutive thirds of every target: the feature table alone (`-t -A`), then
# the same with the feature null of 10 decoys per query, its decoy batch searched under the mask of the targets of its
# owners' kept records (`-t -A -F 10`), and without that mask (PRB_NULL_MASK=0).  Per run the wall time, the records, the
# stage counts of the decoys, and the device time of the stages "feature" (the real batch's fold), "fnull" (the keep, the
# folds, the closes and the gather), "allow" (the mask's test and compaction) and "seed", with the sum of the stages
# behind the seeds.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/fnull_throughput.sh [N=4] [DECOYS=10]
N=${1:-4}
Z=${2:-10}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/fnull_q.fa" "$DB" "$Z" <<'EOF2'
import sys, time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys = int(sys.argv[3])
STAGES = ("fnull", "feature", "allow", "seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3",
          "gapped_slow", "traceback", "traceback_slow", "summary", "raccess")
BEHIND = STAGES[4:15]  # what lies behind the seed stage
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    annot = []
    for p in range(db.npages):
        for i in range(db.page_info(p)[0]):
            length = db.seq_lengths(p, i)[0]
            annot += [(p, i, k * length // 3, (k + 1) * length // 3 - 1) for k in range(3)]
    capi.search_page_summary(ctx, qb, db, 0)  # warm-up (buffers grow to the batch)

    def report(name, wall, extra):
        ms = {s: ctx.stage_ms(s)[0] for s in STAGES}
        print(f"{name}: wall {wall:.3f} s; {extra}; fnull {ms['fnull']:.2f} ms ({ctx.stage_ms('fnull')[1]} launches), feature "
              f"{ms['feature']:.2f} ms ({ctx.stage_ms('feature')[1]} launches), allow {ms['allow']:.1f} ms, seed {ms['seed']:.1f} ms, behind the "
              f"seed stage {sum(ms[s] for s in BEHIND):.1f} ms, raccess {ms['raccess']:.1f} ms")

    with capi.Annotation(ctx, db, annot) as an:
        print(f"{an.count()} features on {an.count() // 3} targets")
        ctx.reset_timers()
        t0 = time.time()
        recs, un = capi.search_features(ctx, qb, db, an)
        report("-t -A", time.time() - t0, f"records {len(recs)}, unassigned {un}")
        tables = {}
        for mask in (True, False):
            ctx.reset_timers()
            t0 = time.time()
            recs = capi.search_fnull(ctx, qb, seqs, db, an, ndecoys, mask=mask)
            tables[mask] = recs
            report(f"-t -A -F {ndecoys}" + ("" if mask else " PRB_NULL_MASK=0"), time.time() - t0,
                   f"records {len(recs)}, NullHits {int(recs['null_hits'].sum())}, NullLE {int(recs['null_le'].sum())}, records with p <= "
                   f"{1.0 / (ndecoys + 1):.3f}: {int((recs['null_le'] == 0).sum())}")
        assert tables[True].tobytes() == tables[False].tobytes(), "the mask changed the table"
        print("the two tables are the same bytes")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/fnull_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each, three features per target" && table
