"""The yardstick of the feature null table (prb_fnullset_*, `ris -t -A FILE -F N`): a plain Python fold by the rules of
include/priblast_hip.h.

For a kept (query q, feature f) record with e_obs = its e_min, and decoy d of q: m(q, d, f) = the minimum e_tot over decoy
d's final hits against f's target whose span shares a position with f - which is the e_min of the record that the feature
table of the decoy (tests/feature_ref.py) has for f -, +infinity without such a hit.  null_hits = the decoys with
m < +infinity, null_le = those with m <= e_obs (compared as floats: -0.0 == +0.0), null_min = the least m (+0.0 for either
zero), +infinity without one.  The fold works from feature records, from lists of hits (through feature_ref.fold), and from
the `-t -A` lines of a real run and of a run of the decoys."""
import math

import numpy as np

import feature_ref


def fold_records(kept, decoy_batches, ndecoys):
    """kept = FEATURE_DTYPE records of the real batch; decoy_batches = [(FEATURE_DTYPE records of a batch of decoys - their
    `query` is the decoy's place in the batch -, owner, decoy)] -> FNULL_DTYPE records in kept's order"""
    from priblast_amd import capi
    m = {}  # (owner, feature) -> {decoy: minimum}
    seen = set()
    for recs, owner, decoy in decoy_batches:
        for k in range(len(owner)):
            assert 0 <= int(decoy[k]) < ndecoys and (int(owner[k]), int(decoy[k])) not in seen
            seen.add((int(owner[k]), int(decoy[k])))
        for r in recs:
            o, d = int(owner[int(r["query"])]), int(decoy[int(r["query"])])
            cell = m.setdefault((o, int(r["feature"])), {})
            assert d not in cell  # (a decoy has one record per feature)
            cell[d] = float(r["e_min"])
    out = np.zeros(len(kept), capi.FNULL_DTYPE)
    for i, r in enumerate(kept):
        for name in capi.FEATURE_DTYPE.names:
            out[i][name] = r[name]
        mins = list(m.get((int(r["query"]), int(r["feature"])), {}).values())
        e_obs = float(r["e_min"])
        out[i]["decoys"] = ndecoys
        out[i]["null_hits"] = len(mins)
        out[i]["null_le"] = sum(1 for x in mins if x <= e_obs)
        out[i]["null_min"] = min(mins) + 0.0 if mins else math.inf
    return out


def fold_hits(real_pages, decoy_batches, annot, seqs, ndecoys):
    """real_pages = {page: (hits, pairs)} of the real batch; decoy_batches = [({page: (hits, pairs)}, owner, decoy)], the hits'
    `query` the decoy's place in its batch; annot and seqs as feature_ref.fold takes them -> FNULL_DTYPE records"""
    kept, _ = feature_ref.fold(real_pages, annot, seqs)
    return fold_records(kept, [(feature_ref.fold(pages, annot, seqs)[0], owner, decoy) for pages, owner, decoy in decoy_batches], ndecoys)


def g6(x):
    """%g of the result lines"""
    return "%g" % x


def fold_lines(real, decoy, decoy_of, ndecoys):
    """real = the `-t -A` lines of the queries' run, decoy = those of the decoys' run (no headers), decoy_of = {decoy's name:
    (query's name, decoy number)} -> the `-t -A -F` lines without their Id.  A feature is known by its target, name and
    range; the energies are the printed ones."""
    m = {}
    for l in decoy:
        f = l.split(",")
        owner, d = decoy_of[f[1]]
        cell = m.setdefault((owner, f[3], f[11], f[12]), {})
        assert d not in cell, l
        cell[d] = float(f[6])
    out = []
    for l in real:
        f = l.split(",")
        mins = list(m.get((f[1], f[3], f[11], f[12]), {}).values())
        le = sum(1 for x in mins if x <= float(f[6]))
        null_min = g6(min(mins) + 0.0) if mins else "NA"
        out.append(",".join(f[1:] + [str(ndecoys), str(len(mins)), str(le), null_min, g6((le + 1.0) / (ndecoys + 1.0))]))
    return out
