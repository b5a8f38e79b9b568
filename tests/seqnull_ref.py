"""The definition of the sequential null table (`ris -t -z N -H H -D R`, include/priblast_hip.h: prb_nullset_retire)
restated in Python, over the per-pair summaries of the real batch and of its decoys.

    boundaries(n, r)                     R, 2R, ... and N
    fold(real, decoys, n, h, r)          the pure part: per boundary b null_ref.fold over the decoys below b, per pair the
                                         record of its Seen - the smallest b with NullLE(b) >= H, or N
    summaries(ctx, qb, seqs, db, n, ...) the summaries taken with capi.search_page_summary - the real batch, then every
                                         decoy in a batch of its own, unmasked -, as fold takes them
"""
import numpy as np

import null_ref
import shuffle_ref


def boundaries(n, r):
    return list(range(r, n, r)) + [n]


def fold(real, decoys, n, h, r, dtype=None):
    """real, decoys: as null_ref.fold takes them, the decoys numbered 0 .. n - 1 -> records by query, then page, then
    db_id; a record's `decoys` is its pair's Seen"""
    assert 1 <= h <= n and 1 <= r <= n
    at = {b: null_ref.fold(real, [x for x in decoys if x[1] < b], b, dtype) for b in boundaries(n, r)}
    out = at[n].copy()
    for i in range(len(out)):
        for b in boundaries(n, r):
            assert (at[b][i]["query"], at[b][i]["page"], at[b][i]["db_id"]) == (out[i]["query"], out[i]["page"], out[i]["db_id"])
            if at[b][i]["null_le"] >= h or b == n:
                out[i] = at[b][i]
                break
    return out


def summaries(ctx, qb, seqs, db, n, seed=1, file_pos=None, opts=None, real_opts=None):
    """-> (real, decoys): {page: records of the real batch}, [(owner, decoy number, {page: records of that decoy})]"""
    from priblast_amd import capi
    file_pos = list(range(len(seqs))) if file_pos is None else list(file_pos)
    real = {p: capi.search_page_summary(ctx, qb, db, p, real_opts or opts) for p in range(db.npages)}
    decoys = []
    for q, s in enumerate(seqs):
        for d in range(n):
            dq = capi.QBatch(ctx, [shuffle_ref.shuffle(s.encode("latin-1"), seed, file_pos[q], d).decode("latin-1")], db.repeat_flag)
            try:
                dq.accessibility(db.W, db.delta)
                decoys.append((q, d, {p: capi.search_page_summary(ctx, dq, db, p, opts) for p in range(db.npages)}))
            finally:
                dq.close()
    return real, decoys


def shows_every_case(real, decoys, n, h, r):
    """What a test's inputs must show, on the reference alone: a pair with Seen at the first boundary, one at a later
    boundary before N, one never retired, and a retired pair whose columns would differ had it gone on to N"""
    seq, full = fold(real, decoys, n, h, r), null_ref.fold(real, decoys, n)
    b = boundaries(n, r)
    never = (seq["decoys"] == n) & (seq["null_le"] < h)
    differs = [(a["null_hits"], a["null_le"], a["null_min"]) != (c["null_hits"], c["null_le"], c["null_min"])
               for a, c in zip(seq, full) if a["decoys"] < n]
    return {"first": bool((seq["decoys"] == b[0]).any() and b[0] < n), "later": bool(((seq["decoys"] > b[0]) & (seq["decoys"] < n)).any()),
            "never": bool(never.any()), "differs": bool(any(differs))}
