#!/bin/bash
# `ris -t -z 10` against `ris -t -z 10 -Q` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb
# queries, one batch through the C ABI, in the manner of null_throughput.sh: the null table finished as it is
# (prb_nullset_finish) and with the Benjamini-Hochberg figures of its pairs ranked on the device (prb_nullset_finish_fdr).
# One warm-up run, then RUNS runs of each: per run the wall time, the queries per second, the observed pairs and the
# device time of the stages "null" (the scatter, the fold, the selection and the gather) and "fdr" (the key pass, the
# sort, the rank pass, the step-up pass and the scatter); the records of the two must be the same bytes.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/fdr_throughput.sh [N=4] [DECOYS=10] [RUNS=3]
N=${1:-4}
Z=${2:-10}
RUNS=${3:-3}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/fdr_q.fa" "$DB" "$Z" "$RUNS" <<'EOF2'
import sys, time
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
ndecoys, runs = int(sys.argv[3]), int(sys.argv[4])
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_null(ctx, qb, seqs, db, ndecoys, fdr=True)  # warm-up (buffers grow to the batch)
    plain = None
    for run in range(runs):
        for fdr in (False, True):
            ctx.reset_timers()
            t0 = time.time()
            got = capi.search_null(ctx, qb, seqs, db, ndecoys, fdr=fdr)
            wall = time.time() - t0
            recs, figs = got if fdr else (got, None)
            if plain is None:
                plain = recs.tobytes()
            assert recs.tobytes() == plain, "the records changed"
            extra = "" if figs is None else f", pairs with QValue < 1: {int((figs['q_den'] != 0).sum()) - int(((figs['q_den'] != 0) & (figs['tests'] * figs['q_num'].astype('i8') == figs['q_den'].astype('i8') * figs['q_rank'])).sum())}"
            print(f"run {run} -t -z {ndecoys}{' -Q' if fdr else ''}: wall {wall:.3f} s, {len(seqs) / wall:.3f} queries/s, pairs {len(recs)}; "
                  f"null {ctx.stage_ms('null')[0]:.3f} ms ({ctx.stage_ms('null')[1]} launches), fdr {ctx.stage_ms('fdr')[0]:.3f} ms "
                  f"({ctx.stage_ms('fdr')[1]} launches){extra}")
    print("the records of every run are the same bytes")
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/fdr_q.fa" &&
  echo "== $N queries of 2 kb, $Z decoys each" && table
