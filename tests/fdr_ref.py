"""The yardstick of `ris -t -z N -Q` and prb_nullset_finish_fdr: the Benjamini-Hochberg figures of a null table's pairs,
from the definition in include/priblast_hip.h, in exact rationals (fractions.Fraction).  Nothing here knows how the
kernels rank: every figure is a count or a minimum over the query's whole list.

A pair is (query, null_le, decoys); its p-value is (null_le + 1) / (decoys + 1).  tests[query] is the number of hypotheses
of its query.  Per pair: rank = the pairs of its query whose p-value is not above its own; FDR = tests * num / (den * rank);
the q-value = min(1, the minimum FDR over the query's pairs whose p-value is not below its own), kept as the minimising
pair's triple (q_num, q_den, q_rank) = (num, den, rank) - among equal fractions the one of lowest rank, then of lowest
den - or (0, 0, 0) when the minimum exceeds 1."""
from fractions import Fraction


def p_key(num, den):
    """the 41-bit integer sort key of the p-value num / den"""
    return (num << 40) // den


def fdr(pairs, tests):
    """pairs = [(query, null_le, decoys)], tests = {query: hypotheses} or a list -> [(tests, rank, q_num, q_den, q_rank)]
    parallel to pairs"""
    frac = [(q, Fraction(le + 1, d + 1), le + 1, d + 1) for q, le, d in pairs]
    by_query = {}
    for i, (q, p, num, den) in enumerate(frac):
        by_query.setdefault(q, []).append(i)
    out = [None] * len(pairs)
    for q, idx in by_query.items():
        ps = sorted(frac[i][1] for i in idx)
        rank = {}
        for i in idx:
            p = frac[i][1]
            lo, hi = 0, len(ps)
            while lo < hi:  # the pairs with p_b <= p
                mid = (lo + hi) // 2
                if ps[mid] <= p:
                    lo = mid + 1
                else:
                    hi = mid
            rank[i] = lo
        t = tests[q]
        # (FDR, rank, den) of every pair, ascending by p; the suffix minimum under that order
        order = sorted(idx, key=lambda i: frac[i][1])
        best, suffix = None, {}
        for i in reversed(order):
            cand = (Fraction(t * frac[i][2], frac[i][3] * rank[i]), rank[i], frac[i][3], frac[i][2])
            if best is None or cand < best:
                best = cand
            suffix[i] = best
        # ... taken at the first pair of each run of equal p-values: every pair of the run sees the whole run
        run_best = {}
        for i in order:
            run_best.setdefault(frac[i][1], suffix[i])
        for i in idx:
            f, r, den, num = run_best[frac[i][1]]
            out[i] = (t, rank[i], 0, 0, 0) if f > 1 else (t, rank[i], num, den, r)
    return out


def q_value(t, q_num, q_den, q_rank):
    """the double that the host prints: 1 for the triple (0, 0, 0), else one division of two exact doubles"""
    return 1.0 if (q_num, q_den, q_rank) == (0, 0, 0) else float(t * q_num) / float(q_den * q_rank)


def columns(fig):
    """(tests, rank, q_num, q_den, q_rank) -> the text of the three columns, without the leading comma"""
    t, rank, q_num, q_den, q_rank = fig
    return "%d,%d,%s" % (t, rank, "%.6g" % q_value(t, q_num, q_den, q_rank))


def brute(pairs, tests):
    """the definition restated pair by pair, O(n^2): no sort, no run, no suffix"""
    out = []
    for qa, lea, da in pairs:
        pa = Fraction(lea + 1, da + 1)
        t = tests[qa]
        mine = [(le + 1, d + 1) for q, le, d in pairs if q == qa]
        rank_of = lambda p: sum(1 for n, d in mine if Fraction(n, d) <= p)
        best = None
        for n, d in mine:
            if Fraction(n, d) >= pa:
                r = rank_of(Fraction(n, d))
                cand = (Fraction(t * n, d * r), r, d, n)
                if best is None or cand < best:
                    best = cand
        out.append((t, rank_of(pa), 0, 0, 0) if best[0] > 1 else (t, rank_of(pa), best[3], best[2], best[1]))
    return out
