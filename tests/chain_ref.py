"""The rule of prb_ris_opts.chain_sites (include/priblast_hip.h) restated in Python, for the tests of `ris -j`: the
yardstick is the plain hit path filtered here, never the selection on the device."""
import numpy as np

from distinct_ref import runs_of


def chains(hits):
    """-> (keep: bool [n], score: float64 [n]): per run an O(L^2) loop in list order.  S(j) = P(j) + e_tot[j]; P(j) = S of
    the hit of lowest S among those that precede j (first of equals), taken only if below 0.0, else 0.0; the chain ends
    at the lowest S (first of equals) and its members are found through the chosen predecessors.  score[i] = S(i)."""
    n = len(hits)
    keep = np.zeros(n, bool)
    q0 = hits["q_sp"].astype(np.int64)
    q1 = q0 + hits["q_len"] - 1
    d0 = hits["db_sp"].astype(np.int64)
    d1 = d0 + hits["db_len"] - 1
    e = hits["e_tot"].astype(np.float64)
    S = np.zeros(n, np.float64)
    prev = np.full(n, -1, np.int64)
    for a, b in runs_of(hits):
        assert (np.diff(d0[a:b]) >= 0).all(), "a run must be sorted by db_sp"
        for j in range(a, b):
            best = -1
            for i in range(a, j):
                if q1[i] < q0[j] and d1[i] < d0[j] and (best < 0 or S[i] < S[best]):  # strict: the first of equals
                    best = i
            P = np.float64(0.0)
            if best >= 0 and S[best] < 0.0:
                P, prev[j] = S[best], best
            S[j] = P + e[j]
        end = a
        for j in range(a + 1, b):
            if S[j] < S[end]:
                end = j
        while end >= 0:
            keep[end] = True
            end = prev[end]
    return keep, S


def keep_mask(hits):
    return chains(hits)[0]


def filter_page(hits, bp):
    """(hits, bp) of prb_search_page without the option -> what it returns with it: the kept records in output order,
    their base-pair lists end to end, bp_offset recomputed; and the keep flags"""
    hits, bp = np.array(hits), np.array(bp).reshape(-1, 2)
    keep = keep_mask(hits)
    out = hits[keep].copy()
    lists = [bp[int(h["bp_offset"]):int(h["bp_offset"]) + int(h["bp_count"])] for h in out]
    out["bp_offset"] = np.concatenate([[0], np.cumsum(out["bp_count"].astype(np.int64))[:-1]]) if len(out) else []
    pairs = np.concatenate(lists).astype(np.int32).reshape(-1, 2) if lists else np.zeros((0, 2), np.int32)
    return out, pairs, keep


def chain_of_each_run(hits):
    """[(a, b, members: indices, score)] per run: the chain's hits and its S"""
    keep, S = chains(hits)
    out = []
    for a, b in runs_of(hits):
        members = a + np.flatnonzero(keep[a:b])
        out.append((a, b, members, S[members[-1]]))
    return out
