"""GPU tests of the per-target coverage table (prb_search_page_coverage, prb_covset_add_hits, `ris -c D`): the regions
of each database sequence that final hits of at least D distinct queries cover.  The yardstick is the contract of
include/priblast_hip.h restated in numpy over prb_search_page's hits: per target the difference arrays, the union of
each (query id, target)'s spans, a backward walk for the first minimum in (energy, query id, place) order, then the
regions by thresholding.  The device records must match it byte for byte."""
import os

import numpy as np
import pytest

import refdump
from test_gpu_options import OPTION_SETS
from test_gpu_targets import RUNS, assert_bytes, open_batch, random_seq, run_ris

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
OPTS = [{}, OPTION_SETS[1], OPTION_SETS[5]]  # defaults; -f -2 -g -5; -m 2


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def seq_info(db):
    """[page][db_id] -> (length, start_pos)"""
    out = []
    for p in range(db.npages):
        nseq, _ = db.page_info(p)
        out.append([(lambda t: (t[0], t[2]))(db.seq_lengths(p, i)) for i in range(nseq)])
    return out


def table(calls, info):
    """The contract restated: calls = [(ids, page, HIT_DTYPE hits of that batch against that page, their pairs)] ->
    {(page, db_id): columns over the sequence's text positions}"""
    per_t = {}
    for ids, page, hits, bp in calls:
        first = {}
        for i, h in enumerate(hits):
            q = int(h["query"])
            first.setdefault(q, i)
            a, b = bp[h["bp_offset"]], bp[h["bp_offset"] + h["bp_count"] - 1]
            L, sp = info[page][int(h["db_id"])]
            lo, hi = min(a[1], b[1]) - sp, max(a[1], b[1]) - sp
            assert 0 <= lo <= hi < L
            e = float(h["e_tot"])
            per_t.setdefault((page, int(h["db_id"])), []).append((e + 0.0, int(ids[q]), i - first[q], lo, hi, e, a, b))
    tab = {}
    for key, hs in per_t.items():
        L = info[key[0]][key[1]][0]
        hdiff, starts, queries = np.zeros(L + 1, np.int64), np.zeros(L, np.int64), np.zeros(L, np.int64)
        seen = {}
        for _, qid, _, lo, hi, _, _, _ in hs:
            hdiff[lo] += 1
            hdiff[hi + 1] -= 1
            starts[lo] += 1
            seen.setdefault(qid, np.zeros(L, bool))[lo:hi + 1] = True  # the union of the pair's spans
        for cov in seen.values():
            queries += cov
        order = sorted(range(len(hs)), key=lambda k: hs[k][:3], reverse=True)  # the walk backward: the lowest writes last
        best = np.full(L, -1, np.int64)
        for k in order:
            best[hs[k][3]:hs[k][4] + 1] = k
        tab[key] = (np.cumsum(hdiff)[:L], starts, queries, best, hs)
    return tab


def max_depth(tab):
    return max([int(t[2].max()) for t in tab.values()] + [0])


def regions(tab, info, d):
    """-> REGION_DTYPE records by page, db_id and start"""
    from priblast_amd import capi
    out = []
    for (page, db_id) in sorted(tab):
        hits, starts, queries, best, hs = tab[(page, db_id)]
        L = info[page][db_id][0]
        deep = np.concatenate([[False], queries >= d, [False]])
        edges = np.flatnonzero(deep[1:] != deep[:-1])
        mine = []
        for a, b in zip(edges[::2], edges[1::2] - 1):  # text positions a..b
            r = np.zeros(1, capi.REGION_DTYPE)[0]
            r["page"], r["db_id"], r["start"], r["end"] = page, db_id, L - 1 - b, L - 1 - a
            r["hits"], r["max_hits"], r["max_queries"] = starts[a:b + 1].sum(), hits[a:b + 1].max(), queries[a:b + 1].max()
            r["peak"] = L - 1 - (a + int(np.flatnonzero(queries[a:b + 1] == queries[a:b + 1].max()).max()))
            h = hs[min(set(best[a:b + 1].tolist()), key=lambda k: hs[k][:3])]
            r["e_min"], r["query"], r["bp_first"], r["bp_last"] = h[5], h[1], h[6], h[7]
            mine.append(r)
        out += sorted(mine, key=lambda r: int(r["start"]))
    return np.array(out, capi.REGION_DTYPE) if out else np.zeros(0, capi.REGION_DTYPE)


def hit_calls(ctx, qb, db, ids, opts=None):
    """-> ([(ids, page, hits, bp)], summed stage counts of the summary search)"""
    from priblast_amd import capi
    calls, counts = [], np.zeros(3, np.int64)
    for p in range(db.npages):
        hits, bp, _ = capi.search_page(ctx, qb, db, p, opts)
        calls.append((ids, p, hits, bp))
        counts += capi.search_page_summary(ctx, qb, db, p, opts, with_counts=True)[1]
    return calls, tuple(int(c) for c in counts)


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    """the mix database (3 pages), its queries as one batch with identifiers 0..nq-1, and their hits (computed once)"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
    qb = open_batch(ctx, db, seqs)
    ids = np.arange(len(seqs), dtype=np.int32)

    class Mix:
        pass
    m = Mix()
    m.names, m.seqs, m.db, m.qb, m.ids, m.info = names, seqs, db, qb, ids, seq_info(db)
    m.calls, m.counts = hit_calls(ctx, qb, db, ids)
    yield m
    qb.close()
    db.close()


def test_coverage_equals_numpy(ctx, golden_dir):
    from priblast_amd import capi
    thinner = 0
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db = capi.Db(ctx, os.path.join(golden_dir, f"{tag}db"))
        qb = open_batch(ctx, db, seqs)
        ids = np.arange(len(seqs), dtype=np.int32)
        info = seq_info(db)
        try:
            for kw in OPTS:
                opts = capi.default_opts(**kw)
                calls, counts = hit_calls(ctx, qb, db, ids, opts)
                tab = table(calls, info)
                most = max_depth(tab)
                want1 = regions(tab, info, 1)
                for d in (1, 2, 3, max(most, 1), most + 1):
                    got, got_counts = capi.search_coverage(ctx, db, d, [(qb, ids)], opts, with_counts=True)
                    assert got_counts == counts
                    want = regions(tab, info, d)
                    print(tag, kw, d, len(got), len(want))
                    assert_bytes(got, want, (tag, kw, d))
                    if d == 2:
                        thinner += want.tobytes() != want1.tobytes()
                assert len(regions(tab, info, most + 1)) == 0
        finally:
            qb.close()
            db.close()
    assert thinner > 0


def test_coverage_does_not_depend_on_batching_or_order(ctx, mix, monkeypatch):
    """one batch; three batches forward and in reverse with identifiers that are a permutation; the pages in reverse; every
    query a sub-batch of its own: the same bytes"""
    from priblast_amd import capi
    db, seqs = mix.db, mix.seqs
    nq = len(seqs)
    perm = np.random.default_rng(11).permutation(nq).astype(np.int32)
    assert not np.array_equal(perm, np.arange(nq))
    cuts = [0, nq // 3, 2 * nq // 3, nq]
    parts = [list(range(cuts[k], cuts[k + 1])) for k in range(3)]
    batches = [(open_batch(ctx, db, [seqs[i] for i in part]), perm[part]) for part in parts]
    try:
        tab = table([(perm, p, h, b) for _, p, h, b in mix.calls], mix.info)
        for d in (1, 2):
            one = capi.search_coverage(ctx, db, d, [(mix.qb, perm)])
            assert_bytes(one, regions(tab, mix.info, d), ("one batch", d))
            assert capi.search_coverage(ctx, db, d, batches).tobytes() == one.tobytes(), d
            assert capi.search_coverage(ctx, db, d, batches[::-1]).tobytes() == one.tobytes(), d
            assert capi.search_coverage(ctx, db, d, batches, pages=list(range(db.npages))[::-1]).tobytes() == one.tobytes(), d
            monkeypatch.setenv("PRB_SEARCH_PAIRS", "1")
            assert capi.search_coverage(ctx, db, d, [(mix.qb, perm)]).tobytes() == one.tobytes(), d
            monkeypatch.delenv("PRB_SEARCH_PAIRS")
    finally:
        for qb, _ in batches:
            qb.close()


def test_coverage_ties_go_by_identifier(ctx, mix):
    """the same query sequence under two identifiers, in different batches, the higher one merged first: wherever that query
    holds a region's best hit, the lower identifier holds it"""
    from priblast_amd import capi
    db, nq = mix.db, len(mix.seqs)
    best = int(np.bincount(regions(table(mix.calls, mix.info), mix.info, 1)["query"], minlength=nq).argmax())
    twin_id = nq + 5
    twin = open_batch(ctx, db, [mix.seqs[best]])
    try:
        twin_ids = np.array([twin_id], np.int32)
        twin_calls, _ = hit_calls(ctx, twin, db, twin_ids)
        tab = table(mix.calls + twin_calls, mix.info)
        for d in (1, 2):
            got = capi.search_coverage(ctx, db, d, [(twin, twin_ids), (mix.qb, mix.ids)])
            assert_bytes(got, regions(tab, mix.info, d), ("twin", d))
            assert (got["query"] == best).any() and not (got["query"] == twin_id).any()
        # the twin doubles the depth wherever the query binds
        assert max_depth(tab) >= 2
    finally:
        twin.close()


# ---- hand-made lists through prb_covset_add_hits ----
HAND_LENS = [1, 63, 64, 65, 300, 50, 64, 64, 300, 200]  # two pages of five sequences; 1,186 slots
HAND_IDS = np.array([7, 3, 9, 1], np.int32)              # (identifier order is not list order)
# (page, query in the list, db_id, first text position, last, e_tot, swapped ends); positions relative to the sequence
HAND_HITS = [
    (0, 0, 0, 0, 0, -9.0, False),      # a one-position region: a whole 1-nt sequence, the first position of the page
    (0, 0, 1, 0, 62, -9.0, False),     # three neighbouring sequences covered from end to end: three regions
    (0, 0, 2, 0, 63, -9.0, False),
    (0, 0, 3, 0, 64, -9.0, True),      # ... of 63, 64 and 65 positions; the last one in the unsorted db0 > dbN form
    (0, 1, 1, 10, 61, -10.0, False),   # depth 2 from text position 10 on
    (0, 2, 1, 62, 62, -11.0, False),   # depth 3 at slot 64 of the page alone: a one-position region of depth 3
    (0, 3, 1, 62, 62, -8.5, False),
    (0, 0, 4, 0, 299, -9.0, False),    # a 300-nt region ...
    (0, 1, 4, 40, 70, -9.0, False),    # ... whose peak is not its first position; across slot 255 / 256
    (1, 3, 1, 5, 20, -9.0, False),     # one pair: two hits that overlap, one that abuts - its query counts once
    (1, 3, 1, 15, 30, -9.5, False),
    (1, 3, 1, 31, 40, -9.0, False),
    (1, 3, 2, 50, 63, -9.0, True),     # up to the last position of a sequence, ends swapped
    (1, 0, 3, 100, 120, -9.5, False),  # two queries with bit-equal e_min: the lower identifier (3, the list's query 1)
    (1, 1, 3, 100, 120, -9.5, False),
    (1, 0, 3, 200, 210, -12.0, False),  # one query, two hits of equal energy on the same positions: the lower place
    (1, 0, 3, 200, 210, -12.0, False),
    (1, 2, 4, 0, 10, 0.0, False),      # +0.0 against -0.0: equal, so identifier 1 (the list's query 3) holds the overlap
    (1, 3, 4, 5, 15, -0.0, False),
    (1, 0, 4, 190, 199, -9.0, False),  # the last position of the page
]                                      # (sequence 0 of page 1 has no hit, between two that have)


@pytest.fixture(scope="module")
def hand(ctx, tmp_path_factory):
    from priblast_amd import capi
    rng = np.random.default_rng(3)
    prefix = str(tmp_path_factory.mktemp("hand") / "handdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(HAND_LENS))], [random_seq(rng, n) for n in HAND_LENS], page_size=5)
    db = capi.Db(ctx, prefix)
    info = seq_info(db)
    assert db.npages == 2 and [L for pg in info for L, _ in pg] == HAND_LENS
    calls = []
    for page in range(2):
        rows = sorted([h for h in HAND_HITS if h[0] == page], key=lambda h: h[1])  # (stable: ascending by query)
        hits, bp = np.zeros(len(rows), capi.HIT_DTYPE), np.zeros((2 * len(rows), 2), np.int32)
        for i, (_, q, d, lo, hi, e, swapped) in enumerate(rows):
            sp = info[page][d][1]
            hits[i]["query"], hits[i]["db_id"], hits[i]["e_tot"], hits[i]["bp_count"], hits[i]["bp_offset"] = q, d, e, 2, 2 * i
            bp[2 * i], bp[2 * i + 1] = (i, sp + (hi if swapped else lo)), (i + 7, sp + (lo if swapped else hi))
        calls.append((HAND_IDS, page, hits, bp))

    class Hand:
        pass
    h = Hand()
    h.db, h.info, h.calls, h.tab = db, info, calls, table(calls, info)
    yield h
    db.close()


def hand_regions(ctx, hand, d, calls=None):
    from priblast_amd import capi
    with capi.CovSet(ctx, hand.db) as cs:
        for ids, page, hits, bp in hand.calls if calls is None else calls:
            cs.add_hits(page, ids, hits, bp)
        assert cs.counts() == (0, 0, 0)
        return cs.finish(d)


def test_hand_made_lists(ctx, hand):
    from priblast_amd import capi
    most = max_depth(hand.tab)
    assert most == 3
    got = {}
    for d in (1, 2, 3, 4):
        got[d] = hand_regions(ctx, hand, d)
        print(d, got[d])
        assert_bytes(got[d], regions(hand.tab, hand.info, d), d)
    assert len(got[4]) == 0
    r1 = got[1]
    def of(page, db_id, recs=r1):
        return recs[(recs["page"] == page) & (recs["db_id"] == db_id)]
    one = of(0, 0)[0]
    assert (int(one["start"]), int(one["end"]), int(one["hits"]), int(one["max_queries"])) == (0, 0, 1, 1)
    for d, L in ((1, 63), (2, 64), (3, 65)):  # whole sequences, each a region of its own
        assert [(int(r["start"]), int(r["end"])) for r in of(0, d)] == [(0, L - 1)]
    assert int(of(0, 1)[0]["max_queries"]) == 3 and int(of(0, 1)[0]["peak"]) == 0  # (text position 62 = forward 0)
    long = of(0, 4)[0]
    assert (int(long["start"]), int(long["end"]), int(long["max_queries"]), int(long["peak"])) == (0, 299, 2, 229)
    assert len(of(1, 0)) == 0
    pair = of(1, 1)[0]  # text 5..40 of a 64-nt sequence
    assert (int(pair["start"]), int(pair["end"]), int(pair["hits"]), int(pair["max_hits"]), int(pair["max_queries"])) == (23, 58, 3, 2, 1)
    assert [(int(r["start"]), int(r["end"])) for r in of(1, 2)] == [(0, 13)]
    tie, place, zero, last = of(1, 3)[1], of(1, 3)[0], of(1, 4)[1], of(1, 4)[0]  # (by forward start: text order reversed)
    assert int(tie["query"]) == 3 and int(tie["max_queries"]) == 2
    assert int(place["query"]) == 7 and int(place["hits"]) == 2
    first_of_pair = [h for h in hand.calls[1][2] if h["db_id"] == 3 and h["e_tot"] == -12.0][0]
    assert place["bp_first"].tolist() == hand.calls[1][3][first_of_pair["bp_offset"]].tolist()
    assert int(zero["query"]) == 1 and zero["e_min"].tobytes() == np.float64(-0.0).tobytes()
    assert (int(last["start"]), int(last["end"])) == (0, 9)
    # depth 2 runs on into the deeper position; depth 3 is that position alone
    assert [(int(r["start"]), int(r["end"])) for r in of(0, 1, got[2])] == [(0, 52)]
    assert [(int(r["start"]), int(r["end"]), int(r["hits"])) for r in of(0, 1, got[3])] == [(0, 0, 2)]
    # the order of the lists does not matter
    assert hand_regions(ctx, hand, 2, hand.calls[::-1]).tobytes() == got[2].tobytes()


def test_span_outside_its_sequence(ctx, hand):
    from priblast_amd import capi
    ids, page, hits, bp = hand.calls[0]
    for shift, which in ((+1, 1), (-1, 0)):  # text 63 of the 63-nt sequence 1 is its separator; before its first position
        bad_bp = bp.copy()
        k = int(np.flatnonzero((hits["db_id"] == 1) & (hits["query"] == 0))[0])
        bad_bp[2 * k + which, 1] += shift
        with capi.CovSet(ctx, hand.db) as cs:
            with pytest.raises(capi.PrbError, match="error -5.*leaves its sequence"):
                cs.add_hits(page, ids, hits, bad_bp)
            cs.add_hits(page, ids, hits, bp)  # (the refused call left the table, and the identifiers, untouched)
            cs.add_hits(1, *hand.calls[1][0:1], *hand.calls[1][2:])
            assert_bytes(cs.finish(1), regions(hand.tab, hand.info, 1), "after the refused list")


def test_covset_merge(ctx, mix, golden_dir):
    from priblast_amd import capi
    db, seqs = mix.db, mix.seqs
    half = len(seqs) // 2
    a_ids, b_ids = mix.ids[:half], mix.ids[half:]
    qa, qbb = open_batch(ctx, db, seqs[:half]), open_batch(ctx, db, seqs[half:])
    other_db = capi.Db(ctx, os.path.join(golden_dir, "c1db"))
    tab = table(mix.calls, mix.info)
    try:
        def fill(which):
            """a table over the (batch, page) sets `which`"""
            cs = capi.CovSet(ctx, db)
            for qb, ids, page in which:
                cs.merge(qb, page, ids)
            return cs
        left = [(qa, a_ids, 0), (qa, a_ids, 1), (qa, a_ids, 2), (qbb, b_ids, 0)]
        right = [(qbb, b_ids, 2), (qbb, b_ids, 1)]
        for d in (1, 2):
            want = regions(tab, mix.info, d)
            for first, second in ((left, right), (right, left)):
                with fill(first) as dst, fill(second) as src:
                    dst.absorb(src)
                    assert dst.counts() == mix.counts
                    assert_bytes(dst.finish(d), want, ("merged", d))
                    assert src.counts() == (0, 0, 0) and len(src.finish(1)) == 0
        # refused merges leave both tables as they were
        want = regions(tab, mix.info, 2)
        with fill(left) as dst, fill(right) as src:
            with fill(right[:1]) as overlap, pytest.raises(capi.PrbError, match="both"):
                src.absorb(overlap)
            with capi.CovSet(ctx, other_db) as foreign, pytest.raises(capi.PrbError, match="different databases"):
                dst.absorb(foreign)
            with pytest.raises(capi.PrbError):
                dst.absorb(dst)
            dst.absorb(src)
            assert_bytes(dst.finish(2), want, "after refused merges")
            with fill([]) as late, pytest.raises(capi.PrbError, match="finished"):
                late.absorb(dst)
    finally:
        qa.close()
        qbb.close()
        other_db.close()


def test_coverage_argument_refusals(ctx, mix, golden_dir):
    from priblast_amd import capi
    db, nq = mix.db, len(mix.seqs)
    other_db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))  # the same files under another handle
    tab = table(mix.calls, mix.info)
    try:
        with capi.CovSet(ctx, db) as cs:
            cs.merge(mix.qb, 1, mix.ids)
            twice = mix.ids.copy()
            twice[1] = twice[0]
            shifted = mix.ids + nq  # fresh identifiers but for the one that is repeated below
            for bad, page, why in ((twice + nq, 0, "twice"), (mix.ids, 1, "already merged"), (-1 - mix.ids, 0, "below 0"),
                                   (np.where(mix.ids == 3, 3, shifted), 1, "already merged")):
                with pytest.raises(capi.PrbError, match=why):
                    cs.merge(mix.qb, page, bad)
            with pytest.raises(capi.PrbError, match="already merged"):
                cs.add_hits(1, mix.ids, *mix.calls[1][2:])
            with pytest.raises(capi.PrbError, match="another database"):
                cs.merge(mix.qb, 0, mix.ids, db=other_db)
            with pytest.raises(capi.PrbError, match="distinct_sites"):
                cs.merge(mix.qb, 0, mix.ids, capi.default_opts(distinct_sites=1))
            with pytest.raises(capi.PrbError, match="unsupported option"):
                cs.merge(mix.qb, 0, mix.ids, capi.default_opts(drop_out_w_gap=31))
            cs.merge(mix.qb, 2, mix.ids)
            cs.add_hits(0, mix.ids, *mix.calls[0][2:])  # (a searched page and a saved list are the same to the table)
            for d in (0, -1, 1000001):
                with pytest.raises(capi.PrbError, match="min_queries"):
                    cs.finish(d)
            got = cs.finish(2)
            assert_bytes(got, regions(tab, mix.info, 2), "after refused calls")
            assert cs.finish(1).tobytes() == got.tobytes()  # (a second call does nothing)
            with pytest.raises(capi.PrbError, match="finished"):
                cs.merge(mix.qb, 0, mix.ids + nq)
    finally:
        other_db.close()


@pytest.mark.parametrize("distinct", [False, True], ids=["all_hits", "distinct_sites"])
def test_cli_region_lines(ctx, mix, golden_dir, tmp_path, distinct):
    from priblast_amd import capi
    u = ["-u"] if distinct else []
    opts = capi.default_opts(distinct_sites=1 if distinct else 0)
    full = run_ris(golden_dir, tmp_path, "t.txt", ["-t"] + u).decode().splitlines(keepends=True)
    header = full[:2] + ["Id,Target name,Target Length,Start,End,Hits,Max Hits,Max Queries,Peak,Minimum Interaction Energy,Query name,"
                         "Query Length,BasePair\n"]
    hits_of = {}
    for l in full[3:]:
        f = l.split(",")
        hits_of[f[3]] = hits_of.get(f[3], 0) + int(f[5])
    qlen = [mix.qb.length_unmasked(q) for q in range(len(mix.seqs))]
    for d in (1, 2):
        recs = capi.search_coverage(ctx, mix.db, d, [(mix.qb, mix.ids)], opts)
        ref = tmp_path / f"ref{d}.txt"
        fd = os.open(str(ref), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        try:
            os.write(fd, "".join(header).encode())
            lines, _ = capi.write_region_lines(mix.db, mix.names, qlen, recs, fd=fd)
        finally:
            os.close(fd)
        assert lines == len(recs) > 0
        want = ref.read_bytes()
        for name, env in RUNS.items():
            assert run_ris(golden_dir, tmp_path, f"c{d}_{name}.txt", ["-c", str(d)] + u, env) == want, (d, name)
        body = want.decode().splitlines(keepends=True)[3:]
        assert [int(l.split(",", 1)[0]) for l in body] == list(range(len(body)))
        if d == 1:
            got_hits = {}
            for l in body:
                f = l.split(",")
                got_hits[f[1]] = got_hits.get(f[1], 0) + int(f[5])
            assert got_hits == hits_of
