"""Device time and launch counts of the stages "summary", "top" and "targets" for one batch of queries against a database,
through the C ABI: once into a top-N table (prb_search_page_top), once into a per-target table
(prb_search_page_targets).  Used by tools/targets_throughput.sh.
usage: targets_stage_times.py QUERIES.fa DBPREFIX N"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from priblast_amd import capi

seqs = "".join(l.strip() if not l.startswith(">") else "\n" for l in open(sys.argv[1])).split()
k = int(sys.argv[3])
ids = np.arange(len(seqs), dtype=np.int32)
with capi.Context(0) as ctx:
    db = capi.Db(ctx, sys.argv[2])
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    capi.search_targets(ctx, db, k, [(qb, ids)])  # warm-up (buffers grow to the batch)
    for name, stage, search in (("top", "top", lambda: capi.search_top(ctx, qb, db, k)),
                                ("targets", "targets", lambda: capi.search_targets(ctx, db, k, [(qb, ids)]))):
        ctx.reset_timers()
        recs = search()
        t, tl = ctx.stage_ms(stage)
        s, sl = ctx.stage_ms("summary")
        print(f"{name} stage: {t:.2f} ms for {len(seqs)} queries ({tl} launches, {len(recs)} records kept); "
              f"summary stage before it: {s:.2f} ms ({sl} launches)")
    qb.close()
    db.close()
