"""The yardstick of the feature table (prb_featset_*, `ris -t -A FILE`): a plain Python fold of final hits into one record
per (query, annotated feature of a target) by the rules of include/priblast_hip.h, and the same fold of `-s 1` text lines
for the command-line tests.

A hit's span on its target is [min(db0, dbN), max(db0, dbN)] of its first and last base pair, in the target's forward
coordinates: length - 1 - (text position - start_pos).  It belongs to every feature (start, end) of its target that the
span shares a position with and is inside the feature when the span lies wholly within it; a hit of no feature is
unassigned.  A record is the `-t` summary over the feature's hits in output order: strict `<` keeps the first minimum,
e_sum is a left-to-right Python float sum from 0.0."""
import math
import re

import numpy as np


def span_of(first_db, last_db, start_pos, length):
    """the forward span of a hit whose first and last pair have the text positions first_db / last_db"""
    a, b = length - 1 - (first_db - start_pos), length - 1 - (last_db - start_pos)
    return min(a, b), max(a, b)


def runs(keys):
    """[(first, behind)] of the maximal runs of equal consecutive keys"""
    out, i = [], 0
    while i < len(keys):
        j = i
        while j < len(keys) and keys[j] == keys[i]:
            j += 1
        out.append((i, j))
        i = j
    return out


def features_of(annot):
    """annot = [(page, db_id, start, end)] -> {(page, db_id): [(start, end, index)] sorted}"""
    by_target = {}
    for i, (p, d, s, e) in enumerate(annot):
        assert 0 <= s <= e
        by_target.setdefault((int(p), int(d)), []).append((int(s), int(e), i))
    for v in by_target.values():
        v.sort()
    return by_target


def fold(pages, annot, seqs):
    """pages = {page: (HIT_DTYPE records in output order, int32 [n, 2] pairs)}; annot = [(page, db_id, start, end)];
    seqs[page][db_id] = (start_pos, length) -> (FEATURE_DTYPE records by query, page, run and feature; unassigned hits)"""
    from priblast_amd import capi
    by_target = features_of(annot)
    rows, unassigned = [], 0
    for page in sorted(pages):
        hits, bp = pages[page]
        bp = np.asarray(bp, np.int32).reshape(-1, 2)
        keys = [(int(h["query"]), int(h["db_id"])) for h in hits]
        assert keys == sorted(keys, key=lambda k: k[0])  # ascending by query
        for a, b in runs(keys):
            q, d = keys[a]
            start_pos, length = seqs[page][d]
            ends, spans = [], []
            for i in range(a, b):
                o, c = int(hits[i]["bp_offset"]), int(hits[i]["bp_count"])
                first, last = bp[o], bp[o + c - 1]
                ends.append((first.tolist(), last.tolist()))
                spans.append(span_of(int(first[1]), int(last[1]), start_pos, length))
                assert 0 <= spans[-1][0] and spans[-1][1] < length
            feats = by_target.get((page, d), [])
            unassigned += sum(1 for lo, hi in spans if not any(lo <= e and hi >= s for s, e, _ in feats))
            for s, e, index in feats:
                n = inside = 0
                e_sum, e_min, best = 0.0, None, -1
                for k, (lo, hi) in enumerate(spans):
                    if lo > e or hi < s:
                        continue
                    x = float(hits[a + k]["e_tot"])
                    e_sum += x
                    if e_min is None or x < e_min:
                        e_min, best = x, k
                    n += 1
                    inside += lo >= s and hi <= e
                if n:
                    h = hits[a + best]
                    rows.append((q, page, (q, d, n, e_min, e_sum, float(h["e_acc"]), float(h["e_hyb"]), ends[best][0], ends[best][1],
                                           page, index, inside)))
    rows.sort(key=lambda r: (r[0], r[1]))  # (stable: runs and features stay in list order)
    out = np.zeros(len(rows), capi.FEATURE_DTYPE)
    for i, (_, _, rec) in enumerate(rows):
        out[i] = rec
    return out, unassigned


PAIR = re.compile(r"\((\d+):(\d+)\)")


def parse_s1(line):
    """a `-s 1` result line with its Id -> (qname, qlen, tname, tlen, e_acc, e_hyb, e_tot as text, [(q, db)] forward pairs)"""
    f = line.split(",")
    pairs = [(int(a), int(b)) for a, b in PAIR.findall(f[8])]
    assert pairs, line
    return f[1], f[2], f[3], f[4], f[5], f[6], f[7], pairs


def fold_lines(lines, annot_of):
    """lines = the result lines of a `ris -s 1` run in its order (no header); annot_of = {target name: [(start, end, name)]} in
    the annotation file's order -> ([the `-t -A` lines without Id and with the Sum column as a float - see line_fields],
    unassigned hits).  The energies are the printed ones: the minimum is taken over their values, first one first."""
    hits = [parse_s1(l) for l in lines]
    out, unassigned = [], 0
    for a, b in runs([(h[0], h[2]) for h in hits]):
        qname, qlen, tname, tlen = hits[a][:4]
        spans = [(min(h[7][0][1], h[7][-1][1]), max(h[7][0][1], h[7][-1][1])) for h in hits[a:b]]
        feats = sorted((s, e, i, name) for i, (s, e, name) in enumerate(annot_of.get(tname, [])))
        unassigned += sum(1 for lo, hi in spans if not any(lo <= e and hi >= s for s, e, _, _ in feats))
        for s, e, _, name in feats:
            members = [k for k, (lo, hi) in enumerate(spans) if lo <= e and hi >= s]
            if not members:
                continue
            best = members[0]
            for k in members:
                if float(hits[a + k][6]) < float(hits[a + best][6]):
                    best = k
            total = 0.0
            for k in members:
                total += float(hits[a + k][6])
            inside = sum(1 for k in members if spans[k][0] >= s and spans[k][1] <= e)
            h = hits[a + best]
            ends = f"({h[7][0][0]}-{h[7][-1][0]}:{h[7][0][1]}-{h[7][-1][1]}) "
            out.append([qname, qlen, tname, tlen, str(len(members)), h[6], total, h[4], h[5], ends, name, f"{s}-{e}", str(inside)])
    return out, unassigned


def line_fields(line):
    """a `-t -A` line with its Id -> the fields of fold_lines (Sum as a float)"""
    f = line.split(",")[1:]
    assert len(f) == 13, line
    f[6] = float(f[6])
    return f


def printed_error(x):
    """half a unit of the sixth significant digit of x: what a printed energy (%g) may be off by"""
    return 0.0 if x == 0 else 0.5 * 10.0 ** (math.floor(math.log10(abs(x))) - 5)


def same_lines(got, want):
    """got = `-t -A` lines of a run, want = fold_lines of its `-s 1` lines: every field equal as text, but the Sum: the
    reference adds printed energies, each off by at most printed_error, and the run prints its own sum, off by as much;
    the bound is worked out per line from those, with the hit count from the line"""
    if len(got) != len(want):
        return False
    for g, w in zip((line_fields(l) for l in got), want):
        if g[:6] != w[:6] or g[7:] != w[7:]:
            return False
        hits = int(w[4])
        # (every energy is negative, so none is larger in magnitude than the minimum, w[5])
        bound = hits * printed_error(float(w[5])) + printed_error(w[6]) + 1e-12
        if abs(g[6] - w[6]) > bound:
            return False
    return True


def golden_annotation(lines):
    """lines = `-s 1` result lines (with or without Id) of a golden output -> [(target name, start, end, feature name)]: an
    annotation built from the hits' own coordinates, so that against these hits it has - by construction - a hit that
    straddles two features, a hit inside a nested feature, a hit that touches a feature by exactly one position at either
    end, an unassigned hit, and a target with hits and no feature (preconditions counts them)"""
    spans = {}  # target -> (length, [(lo, hi)]), by first appearance
    for l in lines:
        f = l.split(",")
        f = f[1:] if len(f) == 9 else f
        pairs = [(int(a), int(b)) for a, b in PAIR.findall(f[7])]
        spans.setdefault(f[2], (int(f[3]), []))[1].append((min(pairs[0][1], pairs[-1][1]), max(pairs[0][1], pairs[-1][1])))
    roles = {"straddle": lambda n, lo, hi: hi > lo, "nested": lambda n, lo, hi: lo > 0 or hi < n - 1, "touch": lambda n, lo, hi: True,
             "away": lambda n, lo, hi: lo > 0, "bare": lambda n, lo, hi: True}
    annot, left = [], dict(roles)
    for t, (n, hits) in spans.items():
        lo, hi = hits[0]
        role = next((r for r, fits in left.items() if fits(n, lo, hi)), None)
        if role is None:
            continue
        del left[role]
        if role == "straddle":
            mid = (lo + hi) // 2
            annot += [(t, 0, mid, "left"), (t, mid + 1, n - 1, "right")]
        elif role == "nested":
            annot += [(t, max(0, lo - 2), min(n - 1, hi + 2), "outer"), (t, lo, hi, "nested")]
        elif role == "touch":
            annot += [(t, hi, min(n - 1, hi + 3), "touch_hi"), (t, max(0, lo - 3), lo, "touch_lo")]
        elif role == "away":
            annot += [(t, 0, 0, "away")]
    assert not left, left
    return annot


def preconditions(lines, annot):
    """how often each of golden_annotation's five conditions holds for the hits of `lines` under `annot`"""
    by_target = {}
    for t, s, e, _ in annot:
        by_target.setdefault(t, []).append((s, e))
    count = dict(straddle=0, nested=0, touch=0, unassigned=0, bare=0)
    bare = set()
    for l in lines:
        f = l.split(",")
        f = f[1:] if len(f) == 9 else f
        pairs = [(int(a), int(b)) for a, b in PAIR.findall(f[7])]
        lo, hi = min(pairs[0][1], pairs[-1][1]), max(pairs[0][1], pairs[-1][1])
        feats = by_target.get(f[2], [])
        mine = [(s, e) for s, e in feats if lo <= e and hi >= s]
        count["straddle"] += len(mine) >= 2 and any(not (lo >= s and hi <= e) for s, e in mine)
        count["nested"] += any(lo >= s and hi <= e and any(s2 <= s and e <= e2 and (s2, e2) != (s, e) for s2, e2 in feats) for s, e in mine)
        count["touch"] += any(min(hi, e) - max(lo, s) == 0 for s, e in mine)
        count["unassigned"] += not mine
        if not feats:
            bare.add(f[2])
    count["bare"] = len(bare)
    return count
