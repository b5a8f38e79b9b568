#!/bin/bash
# `ris -t -A FILE -N 20` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one batch
# through the C ABI, the annotation the three consecutive thirds of every target - the input of fnull_throughput.sh: the
# feature table alone (`-t -A`), the same cut to each query's K best records on the device (`-t -A -N K`), the feature null
# of 10 decoys per query over every record (`-t -A -F 10`) and over the cut (`-t -A -N K -F 10`: the lookup, the scratch
# and the decoys' mask hold the kept records only).  Per run the wall time, the records, and the device time of the stages
# "feature" (the real batch's fold and finish, with the cut's six launches), "fnull", "allow" (the mask's test and
# compaction) and "seed", with the sum of the stages behind the seeds; for the last run its wall time as a fraction of the
# `-F` run's.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/ftop_throughput.sh [N=4] [DECOYS=10] [K=20]
N=${1:-4}
Z=${2:-10}
K=${3:-20}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/fnull_q.fa" "$DB" "$Z" "$K" <<'EOF2'
import sys, time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys, top = int(sys.argv[3]), int(sys.argv[4])
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
        print(f"{name}: wall {wall:.3f} s; {extra}; feature {ms['feature']:.2f} ms ({ctx.stage_ms('feature')[1]} launches), fnull "
              f"{ms['fnull']:.2f} ms ({ctx.stage_ms('fnull')[1]} launches), allow {ms['allow']:.1f} ms, seed {ms['seed']:.1f} ms, behind the "
              f"seed stage {sum(ms[s] for s in BEHIND):.1f} ms, raccess {ms['raccess']:.1f} ms")

    def features(n):
        with capi.FeatSet(ctx, qb, an) as fs:
            for p in range(db.npages):
                fs.merge(db, p)
            return fs.finish() if n is None else fs.finish_top(n)

    with capi.Annotation(ctx, db, annot) as an:
        print(f"{an.count()} features on {an.count() // 3} targets")
        walls = {}
        for n in (None, top):
            ctx.reset_timers()
            t0 = time.time()
            recs = features(n)
            report("-t -A" + ("" if n is None else f" -N {n}"), time.time() - t0, f"records {len(recs)}")
        for n in (None, top):
            ctx.reset_timers()
            t0 = time.time()
            recs = capi.search_fnull(ctx, qb, seqs, db, an, ndecoys, top=n)
            walls[n] = time.time() - t0
            targets = len({(int(p), int(d), int(q)) for p, d, q in zip(recs["page"], recs["db_id"], recs["query"])})
            report("-t -A" + ("" if n is None else f" -N {n}") + f" -F {ndecoys}", walls[n],
                   f"records {len(recs)} on {targets} (query, target) pairs, NullHits {int(recs['null_hits'].sum())}, NullLE {int(recs['null_le'].sum())}")
        print(f"-t -A -N {top} -F {ndecoys} takes {walls[top] / walls[None]:.3f} of the wall time of -t -A -F {ndecoys}")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/fnull_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each, three features per target, the $K best records per query" && table
