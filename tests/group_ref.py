"""The yardstick of the group table (prb_groupset_*, `ris -t -G FILE`): a plain Python fold of per-page pair records into
group records by the rules of include/priblast_hip.h, and the same fold of `-t` text lines for the command-line tests.

A group's record is its best member's pair record: lowest e_min compared as doubles (-0.0 == +0.0), ties to the lower
page, then the lower db_id.  `members` counts the member pairs, `group_hits` sums their hits; nothing else is summed."""
import numpy as np


def fold(pages, maps, ngroups, n=0):
    """pages = {page: PAIR_DTYPE records of the batch against that page}; maps[page][db_id] = group -> GROUP_DTYPE records:
    by query, then group (n = 0); or each query's n groups of lowest (e_min, page, db_id), by query, then rank"""
    from priblast_amd import capi
    best = {}  # (query, group) -> [key, record, page, members, hits]
    for page in sorted(pages):
        for r in pages[page]:
            g = int(maps[page][int(r["db_id"])])
            assert 0 <= g < ngroups
            key = (float(r["e_min"]) + 0.0, page, int(r["db_id"]))  # (-0.0 + 0.0 == +0.0: the two zeros tie)
            slot = best.setdefault((int(r["query"]), g), [key, r, page, 0, 0])
            if key < slot[0]:
                slot[0:3] = [key, r, page]
            slot[3] += 1
            slot[4] += int(r["hits"])
    by_query = {}
    for (q, g), (key, r, page, members, hits) in best.items():
        by_query.setdefault(q, []).append((key, g, r, page, members, hits))
    rows = []
    for q in sorted(by_query):
        if n:
            kept = sorted(by_query[q], key=lambda x: x[0])[:n]
        else:
            kept = sorted(by_query[q], key=lambda x: x[1])
        for rank, (key, g, r, page, members, hits) in enumerate(kept):
            rows.append((r, page, g, members, rank if n else 0, hits))
    out = np.zeros(len(rows), capi.GROUP_DTYPE)
    for i, (r, page, g, members, rank, hits) in enumerate(rows):
        for name in capi.PAIR_DTYPE.names:
            out[i][name] = r[name]
        out[i]["page"], out[i]["group"], out[i]["members"], out[i]["rank"], out[i]["group_hits"] = page, g, members, rank, hits
    return out


def group_numbers(targets, group_of_target):
    """targets = the database's names in database order; group_of_target = {target name: group name} (the -G file) ->
    (group name per target, group names numbered by their first member, targets per group)"""
    names, sizes, of_target = [], {}, []
    for t in targets:
        g = group_of_target.get(t, t)
        if g not in sizes:
            names.append(g)
            sizes[g] = 0
        sizes[g] += 1
        of_target.append(g)
    return of_target, names, sizes


def fold_lines(lines, targets, group_of_target, n=0):
    """lines = the result lines of a `ris -t` run (no header); -> the lines of the same run with -G (and -n N), without
    their Id: the best member's line and ",group,members,targets in the group,hits" behind it"""
    of_target, names, sizes = group_numbers(targets, group_of_target)
    place = {t: i for i, t in reversed(list(enumerate(targets)))}
    number = {g: i for i, g in enumerate(names)}
    queries, best = [], {}
    for line in lines:
        f = line.split(",")
        q, t, hits, e_min = f[1], f[3], int(f[5]), float(f[6])
        if q not in best:
            queries.append(q)
            best[q] = {}
        g = of_target[place[t]]
        key = (e_min + 0.0, place[t])
        slot = best[q].setdefault(g, [key, line, 0, 0])
        if key < slot[0]:
            slot[0:2] = [key, line]
        slot[2] += 1
        slot[3] += hits
    out = []
    for q in queries:
        items = list(best[q].items())
        if n:
            items = sorted(items, key=lambda kv: kv[1][0])[:n]
        else:
            items = sorted(items, key=lambda kv: number[kv[0]])
        for g, (key, line, members, hits) in items:
            out.append(f"{line.split(',', 1)[1]},{g},{members},{sizes[g]},{hits}")
    return out
