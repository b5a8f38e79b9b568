"""The yardstick of the group null table (prb_gnullset_*, `ris -t -G FILE -P N`): the definition of include/priblast_hip.h
restated in plain Python over per-pair summaries of the real batch and of its decoys, and the same fold over `-t` text
lines for the command-line tests.

The observed side is tests/group_ref.py: the kept (query, group) records are those of group_ref.fold(real, maps, ngroups, n).
For a kept (q, g) and decoy d of q, m(q, d, g) = the minimum of the decoy's pair e_min over every target of group g, of any
page, whether or not q itself hit it; +inf without one.  null_hits = #{d: m < inf}, null_le = #{d: m <= e_obs} (doubles:
-0.0 == +0.0), null_min = min m (of the zeros, +0.0).  Decoy records of a group that is not kept for the owner count nowhere."""
import numpy as np

import group_ref


def fold(real, maps, ngroups, decoys, ndecoys, n=0):
    """real: {page: PAIR_DTYPE records of the real batch}; maps[page][db_id] = group; decoys: [(owner, decoy number, {page:
    records of that one decoy, their `query` ignored})] -> GNULL_DTYPE records in the order of group_ref.fold(real, .., n)"""
    from priblast_amd import capi
    kept = group_ref.fold(real, maps, ngroups, n)
    m = {}  # (owner, decoy, group) -> the decoy's minimum over the group's members
    seen = set()
    for owner, d, pages in decoys:
        assert 0 <= d < ndecoys and (owner, d) not in seen
        seen.add((owner, d))
        for page, recs in pages.items():
            ids = [int(x) for x in recs["db_id"]]
            assert len(set(ids)) == len(ids)  # one record per (decoy, target)
            for r in recs:
                key = (int(owner), int(d), int(maps[page][int(r["db_id"])]))
                m[key] = min(m.get(key, np.inf), float(r["e_min"]) + 0.0)  # (-0.0 is reported as +0.0)
    out = np.zeros(len(kept), capi.GNULL_DTYPE)
    for i, k in enumerate(kept):
        for f in capi.GROUP_DTYPE.names:
            out[i][f] = k[f]
        mins = [m.get((int(k["query"]), d, int(k["group"])), np.inf) for d in range(ndecoys)]
        out[i]["decoys"] = ndecoys
        out[i]["null_hits"] = sum(x < np.inf for x in mins)
        out[i]["null_le"] = sum(x <= float(k["e_min"]) for x in mins)
        out[i]["null_min"] = min(mins)
    return out


def p_value(null_le, decoys):
    return (float(null_le) + 1.0) / (float(decoys) + 1.0)


def null_columns(mins, e_obs, ndecoys):
    """the five columns behind a line, from the ndecoys minima (inf: none) of its decoys"""
    hits, le = sum(x < np.inf for x in mins), sum(x <= e_obs for x in mins)
    return "%d,%d,%d,%s,%s" % (ndecoys, hits, le, "%g" % (min(mins) + 0.0) if hits else "NA", "%.6g" % p_value(le, ndecoys))


def fold_lines(real_lines, decoy_lines, decoy_of, targets, group_of_target, ndecoys, n=0):
    """real_lines / decoy_lines = the result lines of `ris -t` runs (no header) on the queries and on a file of their decoys;
    decoy_of = {decoy's name: (its query's name, decoy number)} -> the lines of the queries' run with -G -P ndecoys (and
    -n N), without their Id"""
    of_target, _, _ = group_ref.group_numbers(targets, group_of_target)
    group = dict(zip(targets, of_target))
    m = {}
    for line in decoy_lines:
        f = line.split(",")
        owner, d = decoy_of[f[1]]
        key = (owner, d, group[f[3]])
        m[key] = min(m.get(key, np.inf), float(f[6]) + 0.0)
    out = []
    for line in group_ref.fold_lines(real_lines, targets, group_of_target, n):
        f = line.split(",")
        q, e_obs, g = f[0], float(f[5]), f[-4]
        out.append(line + "," + null_columns([m.get((q, d, g), np.inf) for d in range(ndecoys)], e_obs, ndecoys))
    return out
