#!/bin/bash
# `ris -t -n 20 -G FILE -P 10` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one
# batch through the C ABI, the group map putting five consecutive targets into each group: the 20 best groups per query
# alone (`-t -n 20 -G`), the same with the group null of 10 decoys per query, its decoy batch searched under the mask of
# the members of its owners' kept groups (`-t -n 20 -G -P 10`), and the per-pair null table of every observed pair
# (`-t -z 10`) beside them.  Per run the wall time, the records, the stage counts of the decoys, and the device time of the
# stages "gnull" (the keep, the fold, the close and the gather), "allow" (the mask's test and compaction) and "seed", with
# the sum of the stages behind the seeds.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/gnull_throughput.sh [N=4] [DECOYS=10]
N=${1:-4}
Z=${2:-10}
K=20
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/gnull_q.fa" "$DB" "$Z" "$K" <<'EOF2'
import sys, time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys, k = int(sys.argv[3]), int(sys.argv[4])
STAGES = ("gnull", "group", "null", "allow", "seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3",
          "gapped_slow", "traceback", "traceback_slow", "summary", "raccess")
BEHIND = STAGES[5:16]  # what lies behind the seed stage
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    maps, t = [], 0
    for p in range(db.npages):
        nseq = db.page_info(p)[0]
        maps.append([(t + i) // 5 for i in range(nseq)])
        t += nseq
    ng = (t + 4) // 5
    capi.search_page_summary(ctx, qb, db, 0)  # warm-up (buffers grow to the batch)

    def report(name, wall, extra):
        ms = {s: ctx.stage_ms(s)[0] for s in STAGES}
        print(f"{name}: wall {wall:.3f} s; {extra}; gnull {ms['gnull']:.2f} ms ({ctx.stage_ms('gnull')[1]} launches), group {ms['group']:.2f} ms, "
              f"null {ms['null']:.2f} ms, allow {ms['allow']:.1f} ms, seed {ms['seed']:.1f} ms, behind the seed stage "
              f"{sum(ms[s] for s in BEHIND):.1f} ms, raccess {ms['raccess']:.1f} ms")

    ctx.reset_timers()
    t0 = time.time()
    recs = capi.search_groups(ctx, qb, db, maps, ng, k)
    report(f"-t -n {k} -G", time.time() - t0, f"records {len(recs)} of {ng} groups")
    tables = {}
    for mask in (True, False):
        ctx.reset_timers()
        t0 = time.time()
        recs = capi.search_gnull(ctx, qb, seqs, db, maps, ng, ndecoys, k, mask=mask)
        tables[mask] = recs
        report(f"-t -n {k} -G -P {ndecoys}" + ("" if mask else " PRB_NULL_MASK=0"), time.time() - t0,
               f"records {len(recs)}, NullHits {int(recs['null_hits'].sum())}, NullLE {int(recs['null_le'].sum())}, records with p <= "
               f"{1.0 / (ndecoys + 1):.3f}: {int((recs['null_le'] == 0).sum())}")
    assert tables[True].tobytes() == tables[False].tobytes(), "the mask changed the table"
    print("the two tables are the same bytes")
    ctx.reset_timers()
    t0 = time.time()
    recs, counts, dcounts = capi.search_null(ctx, qb, seqs, db, ndecoys, with_counts=True)
    report(f"-t -z {ndecoys}", time.time() - t0, f"pairs {len(recs)}, decoys {list(dcounts)}, NullHits {int(recs['null_hits'].sum())}")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/gnull_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each, the $K best of the groups of five targets" && table
