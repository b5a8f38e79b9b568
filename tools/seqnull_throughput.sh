#!/bin/bash
# `ris -t -z 100 -H 5 -D 10` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one
# batch through the C ABI: the plain null table with Z decoys per query (`-t -z Z`, its decoy batches under the mask of the
# observed targets) against the sequential one (`-t -z Z -H H -D R`: rounds of R decoys, the pairs that H decoys have
# reached retired on the device after every round, each round under the mask of the pairs still live) and the
# sequential one without a mask (PRB_NULL_MASK=0: only the queries without live pairs are dropped).  Per run the wall
# time, the stage counts of the real batch and of the decoys, the live pairs after each round, the queries dropped, and
# the device time of the stages "null" (scatter, fold, retire, finish), "allow" (the mask's test and compaction, and the
# live mask's kernel) and "seed", with the sum of the stages behind the seeds; and whether the masked and the unmasked
# sequential tables are the same bytes.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/seqnull_throughput.sh [N=4] [Z=100] [H=5] [R=10]
N=${1:-4}
Z=${2:-100}
H=${3:-5}
R=${4:-10}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 1100 python3 - "$W/seqnull_q.fa" "$DB" "$Z" "$H" "$R" <<'EOF2'
import sys, time
import numpy as np
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys, h, per_round = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
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
        print(f"{name}: wall {wall:.3f} s; {extra}; null {ms['null']:.2f} ms ({ctx.stage_ms('null')[1]} launches), allow {ms['allow']:.1f} ms "
              f"({ctx.stage_ms('allow')[1]} launches), seed {ms['seed']:.1f} ms, behind the seed stage {sum(ms[s] for s in BEHIND):.1f} ms, "
              f"raccess {ms['raccess']:.1f} ms", flush=True)

    def columns(recs):
        return (f"pairs {len(recs)}, NullHits {int(recs['null_hits'].sum())}, NullLE {int(recs['null_le'].sum())}, "
                f"pairs with p <= {1.0 / (ndecoys + 1):.4f}: {int(((recs['null_le'] == 0) & (recs['decoys'] == ndecoys)).sum())}")

    ctx.reset_timers()
    t0 = time.time()
    recs, counts, dcounts = capi.search_null(ctx, qb, seqs, db, ndecoys, with_counts=True)
    wall_plain = time.time() - t0
    report(f"-t -z {ndecoys}", wall_plain, f"{columns(recs)}, real {list(counts)}, decoys {list(dcounts)}")
    tables, walls = {}, {}
    for mask in (True, False):
        ctx.reset_timers()
        t0 = time.time()
        recs, counts, dcounts, rounds = capi.search_seqnull(ctx, qb, seqs, db, ndecoys, h, per_round, mask=mask, with_counts=True)
        walls[mask] = time.time() - t0
        tables[mask] = recs
        live = ", ".join(f"{b}: {int(left.sum())}" for b, left in rounds)
        dropped = ", ".join(f"{b}: {int((left == 0).sum())}" for b, left in rounds)
        seen = ", ".join(f"{int(b)}: {int(n)}" for b, n in zip(*np.unique(recs["decoys"], return_counts=True)))
        report(f"-t -z {ndecoys} -H {h} -D {per_round}" + ("" if mask else " PRB_NULL_MASK=0"), walls[mask],
               f"{columns(recs)}, real {list(counts)}, decoys {list(dcounts)}, live pairs after decoy {live}; queries without live pairs after decoy "
               f"{dropped}; pairs by decoys seen {seen}")
    same = tables[True].tobytes() == tables[False].tobytes()
    print("the masked and the unmasked sequential tables are the same bytes" if same else "THE MASK CHANGED THE SEQUENTIAL TABLE")
    print(f"wall time of -t -z {ndecoys} over -t -z {ndecoys} -H {h} -D {per_round}: {wall_plain / walls[True]:.2f} x "
          f"(PRB_NULL_MASK=0: {wall_plain / walls[False]:.2f} x)")
    qb.close()
    db.close()
    sys.exit(0 if same else 1)
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/seqnull_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each, H = $H, rounds of $R" && table
