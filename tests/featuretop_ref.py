"""The yardstick of the ranked cut of the feature table (prb_featset_finish_top, `ris -t -A FILE -N K`): each query's n
best records of a full finish.  The rank key is (e_min, place in the full finish's order); the tests use no zero energies,
so the order of the doubles is the order of the device's energy keys."""
import numpy as np


def select(records, n):
    """records = the FEATURE_DTYPE (or FNULL_DTYPE) records of a full finish, by query ascending -> the first n per query of
    a stable sort by (query, e_min): by query, then rank (a copy)"""
    assert n >= 1 and not (records["e_min"] == 0).any()
    order = sorted(range(len(records)), key=lambda i: (int(records["query"][i]), float(records["e_min"][i])))  # (stable)
    keep, seen = [], {}
    for i in order:
        q = int(records["query"][i])
        if seen.get(q, 0) < n:
            seen[q] = seen.get(q, 0) + 1
            keep.append(i)
    return records[np.array(keep, np.int64)].copy() if keep else records[:0].copy()


def _query_and_energy(line):
    """(query name, printed minimum interaction energy) of a `-t -A` line without its Id"""
    cols = line.split(",")
    return cols[0], float(cols[5])


def select_lines(got, full, n):
    """got = the lines of a `-t -A -N n` run, full = those of the `-t -A` run of the same options, both with their Id ->
    None, or why `got` is not a ranked cut of `full`.  Printed %g energies can tie where the doubles do not, so the order
    within equal printed values is not pinned."""
    if [l.split(",")[0] for l in got] != [str(k) for k in range(len(got))]:
        return "the Ids do not count the written lines"
    got, full = [l.split(",", 1)[1] for l in got], [l.split(",", 1)[1] for l in full]
    of_query, order = {}, []
    for l in full:
        q = _query_and_energy(l)[0]
        if q not in of_query:
            order.append(q)
        of_query.setdefault(q, []).append(l)
    mine = {}
    seen = []
    for l in got:
        q = _query_and_energy(l)[0]
        if q not in of_query or l not in of_query[q]:
            return f"not a line of the full run with the same query: {l}"
        if q in mine and seen[-1] != q:
            return f"the lines of query {q} are not together"
        if q not in mine:
            seen.append(q)
        mine.setdefault(q, []).append(l)
    if seen != [q for q in order if q in mine]:
        return "the queries are not in the full run's order"
    for q, lines in of_query.items():
        kept = mine.get(q, [])
        if len(kept) != min(n, len(lines)):
            return f"query {q}: {len(kept)} lines, want min({n}, {len(lines)})"
        rest = list(lines)
        for l in kept:
            if l not in rest:
                return f"query {q}: a line is written more often than the full run has it"
            rest.remove(l)
        energies = [_query_and_energy(l)[1] for l in kept]
        if any(a > b for a, b in zip(energies, energies[1:])):
            return f"query {q}: the minimum energies decrease with rank: {energies}"
        if rest and min(_query_and_energy(l)[1] for l in rest) < energies[-1]:
            return f"query {q}: a dropped line has a lower energy than the last kept one ({energies[-1]})"
    return None
