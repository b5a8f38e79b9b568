#!/bin/bash
# `ris -k 20 -E 5` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one batch
# through the C ABI: the top-N hit table alone (`-k 20`) against the same table filled beside an evalset
# (prb_search_page_scored), the M decoys per query searched into it (prb_search_page_null_hits), the close and the look-up
# of the kept hits.  Per run the wall time, the stage counts of the real batch and of the decoys, the sizes of the two
# lists, and the device time of the stages "eval" (appends, close, look-up), "tophits", "seed" and "raccess" with the sum
# of the stages behind the seeds; then the close and the look-up on their own.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/eval_throughput.sh [N=4] [DECOYS=5] [K=20]
N=${1:-4}
M=${2:-5}
K=${3:-20}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/eval_q.fa" "$DB" "$M" "$K" <<'EOF2'
import sys, time
import numpy as np
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys, keep = int(sys.argv[3]), int(sys.argv[4])
STAGES = ("eval", "tophits", "seed", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow",
          "traceback", "traceback_slow", "raccess")
BEHIND = STAGES[3:14]  # what lies behind the seed stage
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_tophits(ctx, qb, db, keep)  # warm-up (buffers grow to the batch)

    def report(name, wall, extra):
        ms = {s: ctx.stage_ms(s)[0] for s in STAGES}
        print(f"{name}: wall {wall:.3f} s; {extra}; eval {ms['eval']:.2f} ms ({ctx.stage_ms('eval')[1]} launches), tophits {ms['tophits']:.1f} ms, "
              f"seed {ms['seed']:.1f} ms, behind the seed stage {sum(ms[s] for s in BEHIND):.1f} ms, raccess {ms['raccess']:.1f} ms")

    ctx.reset_timers()
    t0 = time.time()
    alone, alone_bp, counts = capi.search_tophits(ctx, qb, db, keep, with_counts=True)
    report(f"-k {keep}", time.time() - t0, f"kept {len(alone)}, seeds / ungapped / final {list(counts)}")

    ctx.reset_timers()
    t0 = time.time()
    dseqs, owner, decoy = capi.null_decoys(seqs, ndecoys)
    with capi.EvalSet(ctx, qb, db, ndecoys) as es, capi.TopHits(ctx, qb, keep) as th:
        for p in range(db.npages):
            es.scored(p, tophits=th)
        for i0 in range(0, len(dseqs), len(seqs)):  # (decoy batches of the batch's size, as the command line cuts them)
            dqb = capi.QBatch(ctx, dseqs[i0:i0 + len(seqs)], db.repeat_flag)
            try:
                dqb.accessibility(db.W, db.delta)
                for p in range(db.npages):
                    es.null_hits(dqb, p, owner[i0:i0 + len(seqs)], decoy[i0:i0 + len(seqs)])
            finally:
                dqb.close()
        before = ctx.stage_ms("eval")[0]
        t1 = time.time()
        es.finish()
        t_close, ms_close = time.time() - t1, ctx.stage_ms("eval")[0] - before
        recs, bp = th.finish()
        t1 = time.time()
        scores = es.score(recs["query"], recs["e_tot"])
        t_score = time.time() - t1
        nreal, ndec = es.sizes()
        report(f"-k {keep} -E {ndecoys}", time.time() - t0,
               f"kept {len(recs)}, real keys {nreal}, decoy keys {ndec}, real {list(es.counts())}, decoys {list(es.decoy_counts())}, "
               f"lines with NullLE = 0: {int((scores['null_le'] == 0).sum())}, with QValue <= 0.05: "
               f"{int((scores['q_num'] * 20 <= scores['decoys'].astype(np.int64) * scores['q_den']).sum())}")
        print(f"the close: wall {t_close * 1e3:.1f} ms, device {ms_close:.2f} ms; the look-up of {len(recs)} hits: wall {t_score * 1e3:.2f} ms; "
              f"lists at 12 B per key: {(nreal + ndec) * 12 / 2 ** 20:.1f} MB")
    assert recs.tobytes() == alone.tobytes() and bp.tobytes() == alone_bp.tobytes(), "the tee changed the table of -k"
    print("the table of -k is the same bytes")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/eval_q.fa" &&
  echo "== $N queries of 2 kb, $M decoys each, the $K best sites kept" && table
