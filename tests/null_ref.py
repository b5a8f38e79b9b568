"""The definition of the null table (`ris -t -z N`, include/priblast_hip.h) restated in Python, over the per-pair
summaries of the real batch and of its decoys.

    fold(real, decoys, ndecoys)   the pure part: summaries in, NULL_DTYPE records out
    null_ref(ctx, qb, seqs, db, ndecoys, ...)   the summaries taken with capi.search_page_summary - the real batch, then
                                  every decoy (tests/shuffle_ref.py) in a batch of its own, unmasked - and folded
    lines(db, names, qlens, recs) the lines prb_write_null_lines writes, from the `-t` lines of the library
"""
import numpy as np

import shuffle_ref


def null_dtype():
    from priblast_amd import capi
    return capi.NULL_DTYPE


def fold(real, decoys, ndecoys, dtype=None):
    """real: {page: PAIR_DTYPE records of the real batch}; decoys: [(owner, decoy number, {page: records of that one decoy,
    its `query` field ignored})] -> records by query, then page, then db_id."""
    dtype = dtype or null_dtype()
    table = {}  # (query, page, db_id) -> [record, null_hits, null_le, null_min]
    for page, recs in real.items():
        for r in recs:
            key = (int(r["query"]), int(page), int(r["db_id"]))
            assert key not in table
            table[key] = [r, 0, 0, np.inf]
    seen = set()
    for owner, d, pages in decoys:
        assert 0 <= d < ndecoys and (owner, d) not in seen
        seen.add((owner, d))
        for page, recs in pages.items():
            ids = [int(x) for x in recs["db_id"]]
            assert len(set(ids)) == len(ids)  # one record per (decoy, target)
            for r in recs:
                slot = table.get((int(owner), int(page), int(r["db_id"])))
                if slot is None:
                    continue  # an unobserved pair is counted nowhere
                e = float(r["e_min"])
                slot[1] += 1
                slot[2] += e <= float(slot[0]["e_min"])  # (doubles: -0.0 == +0.0)
                slot[3] = min(slot[3], e + 0.0)          # (-0.0 is reported as +0.0)
    out = np.zeros(len(table), dtype)
    for i, key in enumerate(sorted(table)):
        r, nh, nle, nmin = table[key]
        for f in r.dtype.names:
            out[i][f] = r[f]
        out[i]["page"], out[i]["decoys"], out[i]["null_hits"], out[i]["null_le"], out[i]["null_min"] = key[1], ndecoys, nh, nle, nmin
    return out


def null_ref(ctx, qb, seqs, db, ndecoys, seed=1, file_pos0=0, opts=None, with_unobserved=False, file_pos=None, real_opts=None):
    """-> the records; with_unobserved: -> (records, the number of decoy pairs whose (owner, target) is not observed).
    file_pos: every query's place in its file (default: file_pos0 + its index); real_opts: the real batch's options where
    they differ from the decoys' (a pair mask, which belongs to one batch)"""
    from priblast_amd import capi
    file_pos = [file_pos0 + q for q in range(len(seqs))] if file_pos is None else list(file_pos)
    real = {p: capi.search_page_summary(ctx, qb, db, p, real_opts or opts) for p in range(db.npages)}
    observed = {(int(r["query"]), p, int(r["db_id"])) for p, recs in real.items() for r in recs}
    decoys, unobserved = [], 0
    for q, s in enumerate(seqs):
        for d in range(ndecoys):
            dq = capi.QBatch(ctx, [shuffle_ref.shuffle(s.encode("latin-1"), seed, file_pos[q], d).decode("latin-1")], db.repeat_flag)
            try:
                dq.accessibility(db.W, db.delta)
                pages = {p: capi.search_page_summary(ctx, dq, db, p, opts) for p in range(db.npages)}
            finally:
                dq.close()
            unobserved += sum((q, p, int(r["db_id"])) not in observed for p, recs in pages.items() for r in recs)
            decoys.append((q, d, pages))
    recs = fold(real, decoys, ndecoys)
    return (recs, unobserved) if with_unobserved else recs


def p_value(rec):
    return (float(rec["null_le"]) + 1.0) / (float(rec["decoys"]) + 1.0)


def lines(db, names, qlens, recs, id0=0):
    """The `-z` lines of recs: each record's `-t` line as the library writes it (prb_write_summary_lines, pinned by the
    summary tests) with its Id replaced and the null columns behind it, in %g form"""
    import os
    import tempfile
    from priblast_amd import capi
    out = []
    for i, r in enumerate(recs):
        pair = np.zeros(1, capi.PAIR_DTYPE)
        for f in capi.PAIR_DTYPE.names:
            pair[0][f] = r[f]
        pages = [pair if p == int(r["page"]) else np.zeros(0, capi.PAIR_DTYPE) for p in range(db.npages)]
        with tempfile.TemporaryFile() as f:
            capi.write_summary_lines(db, names, qlens, pages, id0=id0 + i, fd=f.fileno())
            f.seek(0)
            line = f.read().decode()
        assert line.endswith("\n") and line.count("\n") == 1
        nmin = "%g" % r["null_min"] if r["null_hits"] > 0 else "NA"
        out.append(line[:-1] + ",%d,%d,%d,%s,%s\n" % (r["decoys"], r["null_hits"], r["null_le"], nmin, "%.6g" % p_value(r)))
    return "".join(out)
