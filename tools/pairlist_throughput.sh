#!/bin/bash
# `ris -L` on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries, one batch through
# the C ABI: the plain search against masks that allow 100 %, 10 % and 1 % of the targets for every query.  Per run the
# wall time of the search, the hit counts and the device time of every stage (prb_ctx_stage_ms), "allow" - the test and
# compaction of the pairs - among them.  Twice: with the default knobs, and with PRB_NO_FRONT_AHEAD=1, where no chunk is
# issued beside the sub-batch before it, so that "seed" and "allow" hold all of their work.
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/pairlist_throughput.sh [N=16]
N=${1:-16}
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
DB=$W/db_s50000x2000
table() {
  (cd "$HERE" && timeout -k 10 900 python3 - "$W/pl_q.fa" "$DB" <<'EOF2'
import sys, time
import numpy as np
from priblast_amd import capi
seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
STAGES = ("seed", "allow", "ungapped", "sort", "filter", "gapped_front", "gapped", "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow",
          "traceback", "traceback_slow")
BEHIND = STAGES[2:]  # what lies behind the seed stage
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    nt = [db.page_info(p)[0] for p in range(db.npages)]
    capi.search_page(ctx, qb, db, 0)  # warm-up (buffers grow to the batch)
    base = None
    for percent in (None, 100, 10, 1):
        mask = None
        if percent is not None:
            mask = capi.PairMask(ctx, qb, db)
            for p, n in enumerate(nt):
                ids = np.arange(0, n, 100 // percent, dtype=np.int32)
                mask.allow(np.full(len(ids), -1), np.full(len(ids), p), ids)
        opts = capi.default_opts(allowed_pairs=mask.h if mask else None)
        ctx.reset_timers()
        t0 = time.time()
        counts = np.zeros(3, np.int64)
        for p in range(db.npages):
            counts += np.array(capi.search_page(ctx, qb, db, p, opts)[2])
        wall = time.time() - t0
        ms = {s: ctx.stage_ms(s)[0] for s in STAGES}
        behind = sum(ms[s] for s in BEHIND)
        base = base or behind
        name = "plain" if percent is None else f"-L {percent} %"
        print(f"{name}: wall {wall:.3f} s; seeds / ungapped / final {counts.tolist()}; behind the seed stage {behind:.1f} ms "
              f"(plain / this = {base / behind:.1f}); " + ", ".join(f"{s} {ms[s]:.1f}" for s in STAGES))
        if mask:
            mask.close()
    qb.close()
    db.close()
EOF2
  )
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/pl_q.fa" &&
  echo "== default knobs, $N queries" && table &&
  echo "== PRB_NO_FRONT_AHEAD=1" && PRB_NO_FRONT_AHEAD=1 table
