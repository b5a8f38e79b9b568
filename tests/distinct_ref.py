"""The rule of prb_ris_opts.distinct_sites (include/priblast_hip.h) restated in Python, for the tests of `ris -u`: the
yardstick is the plain hit path filtered here, never the selection on the device."""
import numpy as np


def runs_of(hits):
    """[(a, b)): the maximal runs of consecutive records with equal (query, db_id)"""
    n = len(hits)
    if n == 0:
        return []
    change = np.flatnonzero((hits["query"][1:] != hits["query"][:-1]) | (hits["db_id"][1:] != hits["db_id"][:-1])) + 1
    edges = [0] + change.tolist() + [n]
    return list(zip(edges[:-1], edges[1:]))


def keep_mask(hits):
    """bool [n]: per run, the hits in the order (e_tot + 0.0, place), each kept iff it intersects no hit kept before it"""
    keep = np.zeros(len(hits), bool)
    q0 = hits["q_sp"].astype(np.int64)
    q1 = q0 + hits["q_len"] - 1
    d0 = hits["db_sp"].astype(np.int64)
    d1 = d0 + hits["db_len"] - 1
    e = hits["e_tot"] + 0.0  # (-0.0 + 0.0 = +0.0: the two compare equal)
    for a, b in runs_of(hits):
        order = a + np.lexsort((np.arange(b - a), e[a:b]))
        kept = np.zeros(0, np.int64)
        for i in order:
            if not ((q0[kept] <= q1[i]) & (q0[i] <= q1[kept]) & (d0[kept] <= d1[i]) & (d0[i] <= d1[kept])).any():
                kept = np.append(kept, i)
        keep[kept] = True
    return keep


def filter_page(hits, bp):
    """(hits, bp) of prb_search_page without the option -> what it returns with it: the kept records in output order,
    their base-pair lists end to end, bp_offset recomputed"""
    hits, bp = np.array(hits), np.array(bp).reshape(-1, 2)
    keep = keep_mask(hits)
    out = hits[keep].copy()
    lists = [bp[int(h["bp_offset"]):int(h["bp_offset"]) + int(h["bp_count"])] for h in out]
    out["bp_offset"] = np.concatenate([[0], np.cumsum(out["bp_count"].astype(np.int64))[:-1]]) if len(out) else []
    pairs = np.concatenate(lists).astype(np.int32).reshape(-1, 2) if lists else np.zeros((0, 2), np.int32)
    return out, pairs, keep


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGU", "UGCA"))


def planted_sequences(seed=5):
    """Queries and targets whose pairs have dense runs of intersecting final hits under `-f -3 -g -6.5`.  Planting the
    reverse complement of a 100-150 nt stretch of a query, with a substitution every 10-20 nt, is not enough: the
    reference (through the CPU oracle) drops 4 % of such a case's hits, because the pieces of a broken duplex lie side by
    side on one diagonal and do not intersect.  Hits that intersect without containing each other lie on NEIGHBOURING
    diagonals, which tandem repeats give: the first query carries 30 copies of a 14 nt unit, the second 4, six targets
    carry 3 to 13 copies of its reverse complement and one 2 kb target 120 (all with a substitution every 10-20 nt), so
    every pair of repeat regions pairs along every diagonal; twelve random 150 nt targets add pairs with one hit or a few.
    On the oracle: 501 hits in 34 pairs, the longest run 106, 2 runs above 64, 23 of 2..63, 9 singletons, 58 % dropped.
    -> (query names, queries, target names, targets)"""
    rng = np.random.default_rng(seed)
    letters = np.array(list("ACGU"))

    def rand(n):
        return "".join(letters[rng.integers(0, 4, n)])

    def mutated(s):
        s, k = list(s), int(rng.integers(10, 21))
        while k < len(s):
            s[k] = letters[(list("ACGU").index(s[k]) + int(rng.integers(1, 4))) % 4]
            k += int(rng.integers(10, 21))
        return "".join(s)

    unit = rand(14)
    queries = [rand(250) + mutated(unit * 30) + rand(200), rand(300) + mutated(unit * 4) + rand(100)]

    def with_repeat(n, units):
        rep = mutated(revcomp(unit) * units)
        at = int(rng.integers(20, max(21, n - len(rep) - 20)))
        s = rand(n)
        return s[:at] + rep + s[at + len(rep):]

    targets = [with_repeat(2000, 120)]
    for t in range(6):
        targets.append(with_repeat(int(rng.integers(500, 1500)), 3 + 2 * t))
    for t in range(12):
        targets.append(rand(150))
    return ["qa", "qb"], queries, [f"t{t}" for t in range(len(targets))], targets
