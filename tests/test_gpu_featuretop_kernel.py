"""GPU tests of the ranked cut of the feature table (prb_featset_finish_top) on hand-made lists through
prb_featset_add_hits: shape A, a 2-page database of 5 + 3 targets of 40 nt and 3 queries, and shape B, 200 targets of
20 nt in pages of 64 and 2 queries, where a query's records fill more than one chunk of the selection.  The yardstick is
featuretop_ref.select over the full finish of an identical second table; records are compared as bytes.  Nothing here
searches: the database and the batch only give the table its shape."""
import numpy as np
import pytest

import featuretop_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1
CHUNK = 2048  # kFtopChunk: the records of one (query, chunk) work item


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def build(ctx, tmp, ntargets, length, page_size, nq):
    from priblast_amd import capi
    rng = np.random.default_rng(23)
    seqs = ["".join(rng.choice(list("ACGU"), length)) for _ in range(ntargets)]
    prefix = str(tmp / "fdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(ntargets)], seqs, page_size=page_size)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(nq)], db.repeat_flag)
    seqs_of = [[(db.seq_lengths(p, i)[2], db.seq_lengths(p, i)[0]) for i in range(db.page_info(p)[0])] for p in range(db.npages)]
    return db, qb, seqs_of


@pytest.fixture(scope="module")
def shape_a(ctx, tmp_path_factory):
    db, qb, seqs = build(ctx, tmp_path_factory.mktemp("ftopdb_a"), 8, 40, 5, 3)
    assert db.npages == 2 and [len(s) for s in seqs] == [5, 3] and all(l == 40 for pg in seqs for _, l in pg)
    yield db, qb, seqs
    qb.close()
    db.close()


@pytest.fixture(scope="module")
def shape_b(ctx, tmp_path_factory):
    db, qb, seqs = build(ctx, tmp_path_factory.mktemp("ftopdb_b"), 200, 20, 64, 2)
    assert [len(s) for s in seqs] == [64, 64, 64, 8]
    yield db, qb, seqs
    qb.close()
    db.close()


def make_hits(rows, seqs_page):
    """rows = [(query, db_id, lo, hi, e_tot)], [lo, hi] the hit's span in forward coordinates -> (HIT_DTYPE records with two
    pairs each, the pairs); every other hit has its first pair at the span's other end, the other fields are recognisable"""
    from priblast_amd import capi
    hits = np.zeros(len(rows), capi.HIT_DTYPE)
    bp = np.zeros((2 * len(rows), 2), np.int32)
    for i, (q, d, lo, hi, e) in enumerate(rows):
        start_pos, length = seqs_page[d]
        t_lo, t_hi = start_pos + length - 1 - hi, start_pos + length - 1 - lo
        first, last = (t_lo, t_hi) if i % 2 else (t_hi, t_lo)
        bp[2 * i], bp[2 * i + 1] = (3 + i % 7, first), (9 + i % 5, last)
        h = hits[i]
        h["query"], h["db_id"], h["e_tot"], h["e_acc"], h["e_hyb"] = q, d, e, 0.125 * i + 1.0, e - 0.125 * i - 1.0
        h["bp_count"], h["bp_offset"] = 2, 2 * i
        h["q_sp"], h["db_sp"], h["q_len"], h["db_len"] = 3, t_lo, 7, hi - lo + 1
    return hits, bp


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def filled(ctx, shape, an, pages, order=None):
    """a feature table with the pages' hits added in `order` (ascending by default); pages = {page: make_hits(...)}"""
    from priblast_amd import capi
    fs = capi.FeatSet(ctx, shape[1], an)
    for p in (order if order is not None else sorted(pages)):
        fs.add_hits(p, *pages[p])
    return fs


def full_finish(ctx, shape, annot, lists):
    from priblast_amd import capi
    pages = {p: make_hits(rows, shape[2][p]) for p, rows in lists.items()}
    with capi.Annotation(ctx, shape[0], annot) as an, filled(ctx, shape, an, pages) as fs:
        return fs.finish()


def top_finish(ctx, shape, annot, lists, n, order=None, split=None):
    """finish_top(n) of the table of `lists`; split = a set of pages that go into a second table, which is merged in"""
    from priblast_amd import capi
    pages = {p: make_hits(rows, shape[2][p]) for p, rows in lists.items()}
    with capi.Annotation(ctx, shape[0], annot) as an:
        if split is None:
            with filled(ctx, shape, an, pages, order) as fs:
                return fs.finish_top(n)
        with filled(ctx, shape, an, {p: v for p, v in pages.items() if p not in split}) as fs, \
                filled(ctx, shape, an, {p: v for p, v in pages.items() if p in split}) as other:
            fs.absorb(other)
            return fs.finish_top(n)


def check(got, full, n):
    want = featuretop_ref.select(full, n)
    assert got.tobytes() == want.tobytes(), (n, got, want)
    return got


# ------------------------------------------------------------------------- shape A: the small cases
# target 1 of page 0 has two features side by side, target 2 of page 1 a nested pair
ANNOT_A = [(0, 0, 0, 39), (0, 1, 0, 19), (0, 1, 20, 39), (0, 3, 5, 30), (1, 0, 0, 39), (1, 2, 10, 20), (1, 2, 0, 39)]
# query 0: 2 records; query 1: 3, two of them - one hit across both features of target 1 - with the same minimum; query 2: 4
LISTS_A = {0: [(0, 0, 1, 5, -5.0), (0, 1, 3, 8, -7.0), (1, 0, 2, 6, -6.5), (1, 1, 18, 22, -4.5), (2, 1, 25, 30, -3.5), (2, 3, 6, 9, -8.0)],
           1: [(2, 0, 1, 2, -9.5), (2, 2, 0, 5, -2.5)]}


@pytest.fixture(scope="module")
def full_a(ctx, shape_a):
    full = full_finish(ctx, shape_a, ANNOT_A, LISTS_A)
    assert [int((full["query"] == q).sum()) for q in range(3)] == [2, 3, 4]
    return full  # computed once, never changed


@pytest.mark.parametrize("n", [1, 2, 3, 4, 1024])
def test_fewer_than_n_exactly_n_and_one_more(ctx, shape_a, full_a, n):
    """n = 3: the queries have n - 1, n and n + 1 records; n = 2 cuts query 1 inside its tie; n = 1; n beyond every count"""
    got = check(top_finish(ctx, shape_a, ANNOT_A, LISTS_A, n), full_a, n)
    assert [int((got["query"] == q).sum()) for q in range(3)] == [min(n, c) for c in (2, 3, 4)]
    if n == 2:  # of the tie at -4.5 the record of the feature that comes first
        assert [(int(r["feature"]), float(r["e_min"])) for r in got[got["query"] == 1]] == [(0, -6.5), (1, -4.5)]
    if n == 1024:  # every record, by rank
        assert sorted(got.tobytes()[i:i + 80] for i in range(0, 80 * len(got), 80)) == sorted(full_a.tobytes()[i:i + 80] for i in range(0, 720, 80))


@pytest.mark.parametrize("without", [0, 1, 2])
def test_a_query_without_a_record(ctx, shape_a, without):
    lists = {p: [r for r in rows if r[0] != without] for p, rows in LISTS_A.items()}
    full = full_finish(ctx, shape_a, ANNOT_A, lists)
    got = check(top_finish(ctx, shape_a, ANNOT_A, lists, 2), full, 2)
    assert not (got["query"] == without).any() and len(got) == sum(min(2, c) for q, c in enumerate((2, 3, 4)) if q != without)


def test_a_table_without_records(ctx, shape_a):
    assert len(top_finish(ctx, shape_a, ANNOT_A, {0: [(1, 2, 0, 5, -3.0)], 1: []}, 3)) == 0  # (target 2 of page 0 has no feature)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_pages_in_both_orders_and_two_tables_merged(ctx, shape_a, full_a, n):
    check(top_finish(ctx, shape_a, ANNOT_A, LISTS_A, n, order=(1, 0)), full_a, n)
    check(top_finish(ctx, shape_a, ANNOT_A, LISTS_A, n, split={1}), full_a, n)
    check(top_finish(ctx, shape_a, ANNOT_A, LISTS_A, n, split={0}), full_a, n)


# an outer feature, a nested one and the outer one again on target 0 of page 0 - one hit inside the nested one is the best
# hit of all three -, a nested pair on target 0 of page 1 with the same minimum, and one lower record on target 1
ANNOT_TIES = [(0, 0, 0, 39), (0, 0, 10, 20), (0, 0, 0, 39), (0, 1, 0, 39), (1, 0, 0, 39), (1, 0, 5, 25)]
LISTS_TIES = {0: [(0, 0, 12, 18, -7.0), (0, 0, 30, 35, -6.0), (0, 1, 3, 4, -9.0)], 1: [(0, 0, 10, 12, -7.0)]}


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_the_cut_inside_a_run_of_equal_minima(ctx, shape_a, n):
    full = full_finish(ctx, shape_a, ANNOT_TIES, LISTS_TIES)
    assert [float(e) for e in full["e_min"]] == [-7.0, -7.0, -7.0, -9.0, -7.0, -7.0] and len(set(full["feature"].tolist())) == 6
    for order in (None, (1, 0)):
        got = check(top_finish(ctx, shape_a, ANNOT_TIES, LISTS_TIES, n, order), full, n)
        # the record at -9, then the ties in the full finish's order: page 0 before page 1, a target's features in theirs
        assert got.tobytes() == full[[3, 0, 1, 2, 4, 5][:n]].tobytes()


# ------------------------------------------------------------------------- shape B: more records than a chunk
# 13 features on every target, overlapping and repeated, that all hold position 10; by their ends a hit at [14, 14] meets 7
# of them and one at [13, 13] meets 8
STARTS = [0, 0, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2]
ENDS = [10, 10, 11, 11, 12, 13, 14, 14, 15, 16, 17, 18, 19]
ANNOT_B = [(t // 64, t % 64, s, e) for t in range(200) for s, e in zip(STARTS, ENDS)]
TIE = range(150, 166)  # the targets whose records (13 each: the places 1950 .. 2157 of query 0) share one minimum


def lists_b(layout, q1_records):
    """query 0: one hit on every target across all its features, the energies a fixed permutation, but for the targets of
    TIE, which share one: the lowest of all ("low"), or one with 70 targets - 910 records, spread over both chunks - below
    it ("mid": rank 1024 then falls among the ties, behind the chunk boundary).  Query 1: q1_records records"""
    perm = np.random.default_rng(5).permutation(200)
    e0 = [-(100.0 + perm[t]) * 0.5 for t in range(200)]  # in [-149.5, -50]
    for t in TIE:
        e0[t] = -200.0 if layout == "low" else -120.25
    if layout == "mid":
        others = [t for t in range(200) if t not in TIE]
        below = {others[i * len(others) // 70] for i in range(70)}
        for t in others:
            e0[t] = -(130.0 + perm[t]) * 0.5 - 60.0 if t in below else -(10.0 + perm[t]) * 0.5
        assert sum(e < -120.25 for e in e0) == 70 and min(below) < 150 and max(below) > 165
    perm1 = np.random.default_rng(6).permutation(158)
    extra = {CHUNK: 14, CHUNK + 1: 13}[q1_records]  # 157 targets x 13 records, and 7 or 8 of target 157
    lists = {p: [] for p in range(4)}
    for q in (0, 1):
        for t in range(200 if q == 0 else 158):
            at = 10 if q == 0 or t < 157 else extra
            lists[t // 64].append((q, t % 64, at, at, e0[t] if q == 0 else -(3.0 + perm1[t]) * 0.25))
    return lists


FULL_B = {}


def full_b(ctx, shape_b, layout, q1_records):
    key = (layout, q1_records)
    if key not in FULL_B:  # computed once per list, never changed
        full = full_finish(ctx, shape_b, ANNOT_B, lists_b(layout, q1_records))
        counts = [int((full["query"] == q).sum()) for q in range(2)]
        assert counts == [2600, q1_records] and counts[0] > CHUNK
        # the ties straddle the chunk boundary
        places = np.flatnonzero(full["e_min"][:2600] == full["e_min"][1950])
        assert places[0] == 1950 and places[-1] == 2157 and len(places) == 208 and places[0] < CHUNK < places[-1]
        FULL_B[key] = full
    return FULL_B[key]


@pytest.mark.parametrize("n", [1, 7, 1024])
@pytest.mark.parametrize("layout,q1_records", [("low", CHUNK), ("mid", CHUNK + 1)])
def test_segments_of_more_than_one_chunk(ctx, shape_b, layout, q1_records, n):
    full = full_b(ctx, shape_b, layout, q1_records)
    got = check(top_finish(ctx, shape_b, ANNOT_B, lists_b(layout, q1_records), n), full, n)
    mine = got[got["query"] == 0]
    assert len(mine) == n and int((got["query"] == 1).sum()) == n
    tie = float(full["e_min"][1950])
    if (layout == "low" and n < 1024) or (layout == "mid" and n == 1024):  # the cut falls inside the run of equal minima
        assert float(mine["e_min"][-1]) == tie and int((full["e_min"][:2600] <= tie).sum()) > n
    if layout == "mid" and n == 1024:  # ... behind the ties of the first chunk: the tie is decided across the chunks
        assert CHUNK - 1950 < int((mine["e_min"] == tie).sum()) < 208
    if n == 1024:  # the kept records come from both chunks (a record of query 0 is known by its feature)
        place = {int(f): i for i, f in enumerate(full["feature"][:2600])}
        kept = [place[int(f)] for f in mine["feature"]]
        assert min(kept) < CHUNK <= max(kept) and sum(k >= CHUNK for k in kept) > 100


def test_chunked_segments_do_not_depend_on_the_page_order_or_a_merge(ctx, shape_b):
    full, lists = full_b(ctx, shape_b, "mid", CHUNK + 1), lists_b("mid", CHUNK + 1)
    check(top_finish(ctx, shape_b, ANNOT_B, lists, 1024, order=(3, 1, 0, 2)), full, 1024)
    check(top_finish(ctx, shape_b, ANNOT_B, lists, 7, split={1, 3}), full, 7)


# ------------------------------------------------------------------------- the guards
def test_a_bad_n_is_refused_and_leaves_the_table(ctx, shape_a, full_a):
    from priblast_amd import capi
    pages = {p: make_hits(rows, shape_a[2][p]) for p, rows in LISTS_A.items()}
    with capi.Annotation(ctx, shape_a[0], ANNOT_A) as an, filled(ctx, shape_a, an, pages) as fs:
        for n in (0, 1025, -1):
            with pytest.raises(capi.PrbError) as e:
                fs.finish_top(n)
            assert code_of(e) == ARG and "1 <= n <= 1024" in str(e.value)
        assert fs.finish().tobytes() == full_a.tobytes()  # a plain finish still works
        with pytest.raises(capi.PrbError) as e:           # ... and is no ranked one
            fs.finish_top(3)
        assert code_of(e) == STATE and "finished" in str(e.value)
        assert fs.finish().tobytes() == full_a.tobytes()


def test_a_table_is_finished_one_way(ctx, shape_a, full_a):
    from priblast_amd import capi
    pages = {p: make_hits(rows, shape_a[2][p]) for p, rows in LISTS_A.items()}
    with capi.Annotation(ctx, shape_a[0], ANNOT_A) as an, filled(ctx, shape_a, an, pages) as fs:
        got = check(fs.finish_top(3), full_a, 3)
        assert fs.finish_top(3).tobytes() == got.tobytes()  # the same n again does nothing
        with pytest.raises(capi.PrbError) as e:
            fs.finish_top(4)
        assert code_of(e) == STATE
        with pytest.raises(capi.PrbError) as e:
            fs.finish()
        assert code_of(e) == STATE
        assert capi.feature_records(fs).tobytes() == got.tobytes()  # the refusals left the records
        with pytest.raises(capi.PrbError) as e:  # nothing is merged after it
            fs.add_hits(0, *pages[0])
        assert code_of(e) == STATE


def test_the_stage_timer_counts_the_selection(ctx, shape_a):
    pages = {p: make_hits(rows, shape_a[2][p]) for p, rows in LISTS_A.items()}
    from priblast_amd import capi
    with capi.Annotation(ctx, shape_a[0], ANNOT_A) as an:
        counts = []
        for n in (None, 2):
            with filled(ctx, shape_a, an, pages) as fs:
                ctx.reset_timers()
                fs.finish() if n is None else fs.finish_top(n)
                counts.append(ctx.stage_ms("feature")[1])
    assert counts == [3, 9]  # the cells' counts, their scan and the gather; behind them the six launches of the cut
