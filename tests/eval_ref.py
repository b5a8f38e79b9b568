"""A plain restatement of the evalset's definitions (include/priblast_hip.h, `ris -k N -E M`): sort, count, and
fractions.Fraction for the minimum.  For one query with the energies `real` of its final hits and `decoy` of the pooled
hits of its M decoys, per real hit h:

    rank     real hits with energy <= h's (h included; -0.0 == +0.0)
    null_le  decoy hits with energy <= h's
    FDR_g    null_le_g / (M * rank_g)
    q        min(1, min of FDR_g over the real hits g with energy >= h's), kept as (q_num, q_den) = (null_le_g, rank_g) of the
             minimising g - among equal fractions the g of lowest energy -, or (M, 1) when the minimum exceeds 1

Nothing here is shared with the library: numpy's sort and searchsorted on the doubles, Python's exact rationals."""
from fractions import Fraction

import numpy as np

DTYPE = np.dtype([("decoys", "<i8"), ("null_le", "<i8"), ("rank", "<i8"), ("q_num", "<i8"), ("q_den", "<i8")])


def score_query(real, decoy, ndecoys):
    """-> DTYPE records, one per entry of `real`, in its order"""
    real = np.asarray(real, np.float64) + 0.0  # (-0.0 -> +0.0)
    decoy = np.sort(np.asarray(decoy, np.float64) + 0.0)
    out = np.zeros(len(real), DTYPE)
    if not len(real):
        return out
    srt = np.sort(real)
    out["decoys"] = ndecoys
    out["rank"] = np.searchsorted(srt, real, side="right")
    out["null_le"] = np.searchsorted(decoy, real, side="right")
    # the distinct energies, ascending, with their (null_le, rank); the suffix minimum from the highest one down
    levels = np.unique(srt)
    nle = np.searchsorted(decoy, levels, side="right")
    rank = np.searchsorted(srt, levels, side="right")
    best = [None] * len(levels)
    cur = None
    for k in range(len(levels) - 1, -1, -1):
        f = Fraction(int(nle[k]), int(ndecoys) * int(rank[k]))
        if cur is None or f <= cur[0]:  # (an equal fraction goes to the lower energy)
            cur = (f, int(nle[k]), int(rank[k]))
        best[k] = cur
    at = np.searchsorted(levels, real)
    for i, k in enumerate(at):
        f, n, r = best[k]
        out["q_num"][i], out["q_den"][i] = (ndecoys, 1) if f > 1 else (n, r)
    return out


def score(nq, real_q, real_e, decoy_owner, decoy_e, ndecoys, look_q=None, look_e=None):
    """The records of the hits (look_q[i], look_e[i]) - by default of every real hit, in the lists' order - for a batch of nq
    queries with the real hits (real_q, real_e) and the decoy hits (decoy_owner, decoy_e)."""
    real_q, real_e = np.asarray(real_q, np.int64), np.asarray(real_e, np.float64)
    decoy_owner, decoy_e = np.asarray(decoy_owner, np.int64), np.asarray(decoy_e, np.float64)
    look_q = real_q if look_q is None else np.asarray(look_q, np.int64)
    look_e = real_e if look_e is None else np.asarray(look_e, np.float64)
    out = np.zeros(len(look_q), DTYPE)
    for q in range(nq):
        mine = real_e[real_q == q]
        recs = score_query(mine, decoy_e[decoy_owner == q], ndecoys)
        for i in np.nonzero(look_q == q)[0]:
            hit = np.nonzero(mine + 0.0 == look_e[i] + 0.0)[0]
            assert len(hit), f"query {q} has no real hit of energy {look_e[i]}"
            out[i] = recs[hit[0]]
    return out


def evalue(rec):
    return rec["null_le"] / rec["decoys"]


def qvalue(rec):
    return rec["q_num"] / (rec["decoys"] * rec["q_den"])
