"""GPU tests of the table merges (prb_topset_merge, prb_tophits_merge, prb_profset_merge): two unfinished tables over
disjoint page sets of one batch become the one table that took all those pages directly - byte for byte, stage counts
included - and the table merged from is left empty.  The yardstick is the table filled page by page under one context
(pinned to the summary and hit paths by test_gpu_top.py, test_gpu_tophits.py and test_gpu_profile.py).

Shapes: three pages of 300 random 300-nt targets; three queries of 600-900 nt, the last one poly-A, which has no hit
under -g -9.  A query has up to 300 pairs per page - some hundred of them with a hit - so n = 1 and 3 cut every list,
n = 70 is more than a wavefront's worth of slots, and n = 1024 leaves the lists short and is the size at which a
workgroup writes back in four rounds of 256 places."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 3, 70, 1024)
KINDS = ("top", "tophits0", "tophits1")
CASES = [(k, n) for k in KINDS for n in NS] + [("profile", 0)]
STRICT = dict(final_threshold=-9.0)


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


class World:
    """two contexts on device 0, each with its own handle of the database and its own batch of the same queries - what
    two workers of the command line hold - and the tables taken directly, computed once per (kind, n)"""

    def __init__(self, tmp, targets_of_page, queries, tag):
        from priblast_amd import capi
        self.capi = capi
        self.ctx = [capi.Context(0), capi.Context(0)]
        prefix = str(tmp / tag)
        seqs = [s for page in targets_of_page for s in page]
        capi.db_build(self.ctx[0], prefix, [f"t{i}" for i in range(len(seqs))], seqs, page_size=len(targets_of_page[0]))
        self.db = [capi.Db(c, prefix) for c in self.ctx]
        assert self.db[0].npages == len(targets_of_page)
        self.qb = []
        for c, db in zip(self.ctx, self.db):
            qb = capi.QBatch(c, queries, db.repeat_flag)
            qb.accessibility(db.W, db.delta)
            self.qb.append(qb)
        self.queries = queries
        self._direct = {}

    def close(self):
        for x in self.qb + self.db + self.ctx:
            x.close()

    def opts(self, kind, **kw):
        return self.capi.default_opts(output_style=1 if kind == "tophits1" else 0, **kw)

    def table(self, kind, n, who, pages, qb=None, **kw):
        """an unfinished table of `kind` under context `who` with `pages` merged into it"""
        capi = self.capi
        ctx, qb = self.ctx[who], qb or self.qb[who]
        t = capi.TopSet(ctx, qb, n) if kind == "top" else capi.ProfSet(ctx, qb) if kind == "profile" else capi.TopHits(ctx, qb, n)
        for p in pages:
            t.merge(self.db[who], p, self.opts(kind, **({**STRICT, **kw})))
        return t

    def direct(self, kind, n, pages=(0, 1, 2)):
        key = (kind, n, tuple(pages))
        if key not in self._direct:
            with self.table(kind, n, 0, pages) as t:
                self._direct[key] = finished(t)
        return self._direct[key]


def finished(t):
    """finish -> (the bytes of every array the table gives, the stage counts)"""
    out = t.finish()
    arrays = out if isinstance(out, tuple) else (out,)
    return tuple(a.tobytes() for a in arrays), t.counts(), arrays


def assert_same(got, want, what):
    assert got[1] == want[1], (what, "counts", got[1], want[1])
    for k, (a, b) in enumerate(zip(got[2], want[2])):
        assert len(a) == len(b), (what, k, len(a), len(b))
        if a.tobytes() != b.tobytes():
            for i in range(len(a)):
                assert a[i].tobytes() == b[i].tobytes(), (what, k, i, a[i], b[i])
    assert got[0] == want[0], what


def assert_empty(t, what):
    got = finished(t)
    assert got[1] == (0, 0, 0) and all(len(a) == 0 for a in got[2]), (what, got[1], [len(a) for a in got[2]])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    rng = np.random.default_rng(11)
    pages = [[random_seq(rng, 300) for _ in range(300)] for _ in range(3)]
    queries = [random_seq(rng, 900), random_seq(rng, 600), "A" * 700]
    w = World(tmp_path_factory.mktemp("mergedb"), pages, queries, "rand")
    yield w
    w.close()


@pytest.fixture(scope="module")
def tie_world(tmp_path_factory):
    """the same 40 targets in each of the three pages: every record has two twins of bit-identical energy in the other
    pages, so records of equal energy meet from different tables at every rank"""
    rng = np.random.default_rng(12)
    page = [random_seq(rng, 300) for _ in range(40)]
    queries = [random_seq(rng, 800), random_seq(rng, 600)]
    w = World(tmp_path_factory.mktemp("tiedb"), [page, page, page], queries, "tie")
    yield w
    w.close()


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_merge_page_splits(world, kind, n):
    w = world
    want = w.direct(kind, n)
    recs = want[2][0]
    assert len(recs) > 0 and 2 not in set(recs["query"].tolist())  # (the poly-A query has no hit)
    if kind != "profile":
        per_q = np.bincount(recs["query"], minlength=3)
        print(kind, n, "records per query:", per_q.tolist())
        if n <= 3:
            assert per_q[0] == n and per_q[1] == n, per_q  # (cut lists)
        if n == 70:
            assert per_q[0] > 64, per_q  # (a list longer than a wavefront)
        if kind == "top" and n == 1024:
            assert 0 < per_q[0] < n and 0 < per_q[1] < n, per_q  # (short lists: 900 targets in all)
    # {0} <- {1} <- {2}: tables of two contexts
    t0, t1, t2 = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [1]), w.table(kind, n, 0, [2])
    with t0, t1, t2:
        t0.absorb(t1)
        t0.absorb(t2)
        assert_same(finished(t0), want, (kind, n, "0<-1<-2"))
        assert_empty(t1, "src 1")
        assert_empty(t2, "src 2")
    # {2} <- {0} <- {1}: another order, the other context
    t0, t1, t2 = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [1]), w.table(kind, n, 1, [2])
    with t0, t1, t2:
        t2.absorb(t0)
        t2.absorb(t1)
        assert_same(finished(t2), want, (kind, n, "2<-0<-1"))
    # {0, 2} <- {1}
    a, b = w.table(kind, n, 0, [0, 2]), w.table(kind, n, 1, [1])
    with a, b:
        a.absorb(b)
        assert_same(finished(a), want, (kind, n, "02<-1"))


@pytest.mark.parametrize("kind,n", [("top", 1), ("top", 50), ("tophits0", 2), ("tophits1", 50), ("profile", 0)])
def test_merge_ties_come_out_in_page_order(tie_world, kind, n):
    w = tie_world
    want = w.direct(kind, n)
    recs = want[2][0]
    assert len(recs) > 0
    if kind == "profile":
        assert set(recs["page"].tolist()) == {0}  # (the best hit's twins in pages 1 and 2 lose the tie)
    else:
        e = recs["e_min" if kind == "top" else "e_tot"].view(np.uint64)
        q, pg = recs["query"], recs["page"]
        ties = [(i, i + 1) for i in range(len(recs) - 1) if q[i] == q[i + 1] and e[i] == e[i + 1]]
        assert (n == 1 or ties) and all(pg[i] <= pg[j] for i, j in ties), ties
        if n == 1:
            assert set(pg.tolist()) == {0}
    for order in ([2, 1, 0], [1, 0, 2]):
        tabs = [w.table(kind, n, k % 2, [p]) for k, p in enumerate(order)]
        try:
            tabs[0].absorb(tabs[1])
            tabs[0].absorb(tabs[2])
            assert_same(finished(tabs[0]), want, (kind, n, order))
        finally:
            for t in tabs:
                t.close()


@pytest.mark.parametrize("kind,n", [("top", 3), ("tophits1", 3), ("profile", 0)])
def test_merge_of_an_empty_table_changes_nothing(world, kind, n):
    w = world
    want = w.direct(kind, n, (0, 1))
    full, empty = w.table(kind, n, 0, [0, 1]), w.table(kind, n, 1, [])
    with full, empty:
        full.absorb(empty)
        assert_same(finished(full), want, (kind, "empty src"))
        assert_empty(empty, "empty src")
    full, empty = w.table(kind, n, 0, [0, 1]), w.table(kind, n, 1, [])
    with full, empty:
        empty.absorb(full)
        assert_same(finished(empty), want, (kind, "empty dst"))
        assert_empty(full, "emptied src")


@pytest.mark.parametrize("kind", ["top", "tophits1", "profile"])
def test_merge_refusals_leave_both_tables_alone(world, kind):
    w, capi = world, world.capi
    n = 3
    want0, want1 = w.direct(kind, n, (0,)), w.direct(kind, n, (0, 1))

    def refused(dst, src, text):
        with pytest.raises(capi.PrbError) as err:
            dst.absorb(src)
        assert "error -1" in str(err.value) and text in str(err.value), err.value

    # overlapping page sets
    a, b = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [0, 1])
    with a, b:
        refused(a, b, "page 0 is merged into both")
        assert_same(finished(a), want0, (kind, "overlap dst"))
        assert_same(finished(b), want1, (kind, "overlap src"))
    # a finished table, in either role
    a, b = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [1])
    with a, b:
        assert_same(finished(a), want0, kind)
        refused(a, b, "finished")
        refused(b, a, "finished")
        assert_same(finished(a), want0, (kind, "finished"))
        assert_same(finished(b), w.direct(kind, n, (1,)), (kind, "beside finished"))
    # another number of queries, other lengths
    for other in (w.queries[:2], [w.queries[0], w.queries[1] + "A", w.queries[2]]):
        qb = capi.QBatch(w.ctx[1], other, w.db[1].repeat_flag)
        qb.accessibility(w.db[1].W, w.db[1].delta)
        try:
            a, b = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [], qb=qb)
            with a, b:
                refused(a, b, "queries")
                refused(b, a, "queries")
                assert_same(finished(a), want0, (kind, "queries"))
                assert_empty(b, "queries")
        finally:
            qb.close()
    if kind != "profile":  # different n
        a, b = w.table(kind, n, 0, [0]), w.table(kind, n + 1, 1, [1])
        with a, b:
            refused(a, b, "records per query")
            assert_same(finished(a), want0, (kind, "n"))
            assert_same(finished(b), w.direct(kind, n + 1, (1,)), (kind, "n src"))
    if kind == "tophits1":  # mixed -k styles; a table without a page has no style yet
        a, b = w.table("tophits1", n, 0, [0]), w.table("tophits0", n, 1, [1])
        with a, b:
            refused(a, b, "output_style")
            assert_same(finished(a), want0, (kind, "style"))
            assert_same(finished(b), w.direct("tophits0", n, (1,)), (kind, "style src"))


@pytest.mark.parametrize("style", [0, 1])
def test_merged_tophits_pool_is_gap_free_and_true(world, style):
    """the merged table's pair lists lie in record order without gaps, and each is its hit's list from prb_search_page"""
    w, capi = world, world.capi
    kind, n = f"tophits{style}", 70
    t0, t1, t2 = w.table(kind, n, 0, [0]), w.table(kind, n, 1, [1]), w.table(kind, n, 0, [2])
    with t0, t1, t2:
        t1.absorb(t2)
        t1.absorb(t0)
        recs, bp = t1.finish()
    print(f"tophits{style}: {len(recs)} records, {len(bp)} pairs")
    assert len(recs) > 3 and set(recs["page"].tolist()) == {0, 1, 2}
    assert recs["bp_offset"].tolist() == (np.cumsum(recs["bp_count"]) - recs["bp_count"]).tolist()
    assert int(recs["bp_count"].sum()) == len(bp)
    key = ["query", "q_sp", "db_sp", "q_len", "db_len", "db_id"]
    for page in range(3):
        hits, hbp, _ = capi.search_page(w.ctx[0], w.qb[0], w.db[0], page, w.opts(kind, **STRICT))
        where = {tuple(int(h[f]) for f in key): i for i, h in enumerate(hits)}
        for r in recs[recs["page"] == page]:
            h = hits[where[tuple(int(r[f]) for f in key)]]
            for f in ("e_acc", "e_hyb", "e_tot", "bp_count", "db_id_start"):
                assert r[f] == h[f], (page, f, r, h)
            mine = bp[int(r["bp_offset"]):int(r["bp_offset"]) + int(r["bp_count"])]
            theirs = hbp[int(h["bp_offset"]):int(h["bp_offset"]) + int(h["bp_count"])]
            assert mine.tobytes() == theirs.tobytes(), (page, r)
