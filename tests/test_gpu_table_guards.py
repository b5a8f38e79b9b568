"""GPU tests of what the five result tables refuse (prb_topset_*, prb_tophits_*, prb_profset_*, prb_targetset_*,
prb_covset_*): the error code and the whole error text of every refused merge and finish, the order of the checks where
a call breaks two conditions at once, and that a refused call leaves every table involved as it was - it still
finishes to what it would have held without the call.  The texts are spelled out here; what the tables hold is pinned
by test_gpu_top.py, test_gpu_tophits.py, test_gpu_profile.py, test_gpu_targets.py, test_gpu_coverage.py and
test_gpu_merge.py.

Shapes: the c1 golden targets (32) built as two pages of 16 under two contexts of device 0, three of the c1 queries; a
second database of 20 of those targets in two pages of 10 for the tables "of another shape"."""
import contextlib
import os

import numpy as np
import pytest

import refdump

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("top", "tophits", "profile", "targets", "coverage")
BATCH, RUN = KINDS[:3], KINDS[3:]
PREFIX = dict(top="topset", tophits="tophits", profile="profset", targets="targetset", coverage="covset")
NOUN = dict(top="top-N", tophits="top-N hit", profile="profile", targets="per-target", coverage="coverage")
N, DEPTH = 3, 1
IDS = (0, 1, 2)
ARG, STATE = -1, -5


class World:
    """two contexts on device 0, each with its own handle of the two databases and its own batch of the same queries"""

    def __init__(self, tmp):
        from priblast_amd import capi
        self.capi = capi
        names, targets = refdump.read_fasta(os.path.join(GOLDEN, "c1_db.fa"))
        _, queries = refdump.read_fasta(os.path.join(GOLDEN, "c1_q.fa"))
        self.ctx = [capi.Context(0), capi.Context(0)]
        capi.db_build(self.ctx[0], str(tmp / "c1"), names, targets, page_size=16)
        capi.db_build(self.ctx[0], str(tmp / "small"), names[:20], targets[:20], page_size=10)
        self.db = [capi.Db(c, str(tmp / "c1")) for c in self.ctx]
        self.small = capi.Db(self.ctx[1], str(tmp / "small"))
        assert self.db[0].npages == 2 and self.small.npages == 2
        self.qb = []
        for c, db in zip(self.ctx, self.db):
            qb = capi.QBatch(c, queries[:3], db.repeat_flag)
            qb.accessibility(db.W, db.delta)
            self.qb.append(qb)
        self._direct = {}

    def close(self):
        for x in self.qb + self.db + [self.small] + self.ctx:
            x.close()

    def opts(self, style=1, distinct=0):
        return self.capi.default_opts(output_style=style, distinct_sites=distinct)

    def empty(self, kind, who, n=N, db=None):
        capi, ctx = self.capi, self.ctx[who]
        if kind == "top":
            return capi.TopSet(ctx, self.qb[who], n)
        if kind == "tophits":
            return capi.TopHits(ctx, self.qb[who], n)
        if kind == "profile":
            return capi.ProfSet(ctx, self.qb[who])
        if kind == "targets":
            return capi.TargetSet(ctx, db or self.db[who], n)
        return capi.CovSet(ctx, db or self.db[who])

    def add(self, kind, t, who, page, ids=IDS, **kw):
        """page `page` searched under context `who` and merged into t"""
        if kind in BATCH:
            t.merge(self.db[who], page, self.opts(**kw))
        else:
            t.merge(self.qb[who], page, ids, self.opts(**kw), db=self.db[who])

    def table(self, kind, who, pages, n=N, **kw):
        t = self.empty(kind, who, n)
        for p in pages:
            self.add(kind, t, who, p, **kw)
        return t

    def direct(self, kind, pages, n=N, **kw):
        key = (kind, tuple(pages), n, tuple(sorted(kw.items())))
        if key not in self._direct:
            with self.table(kind, 0, pages, n, **kw) as t:
                self._direct[key] = finished(kind, t)
        return self._direct[key]


def finished(kind, t):
    """finish -> (the bytes of every array the table gives, the stage counts)"""
    out = t.finish(DEPTH) if kind == "coverage" else t.finish()
    arrays = out if isinstance(out, tuple) else (out,)
    return tuple(a.tobytes() for a in arrays), t.counts()


@contextlib.contextmanager
def through(t, ctx):
    """t's calls go through the context `ctx`"""
    own, t.ctx = t.ctx, ctx
    try:
        yield t
    finally:
        t.ctx = own


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("guarddb"))
    yield w
    w.close()


def refused(w, call, code, text):
    with pytest.raises(w.capi.PrbError) as err:
        call()
    assert str(err.value) == f"libpriblast_hip error {code}: {text}"


@pytest.mark.parametrize("kind", KINDS)
def test_direct_tables_hold_something(world, kind):
    w = world
    for pages in ((0,), (1,), (0, 1)):
        arrays, counts = w.direct(kind, pages)
        assert len(arrays[0]) > 0 and counts[2] > 0, (kind, pages, counts)
    assert w.direct(kind, (0,)) != w.direct(kind, (0, 1))


@pytest.mark.parametrize("kind", KINDS)
def test_refused_table_merges(world, kind):
    w, fn, tables = world, f"prb_{PREFIX[kind]}_merge", f"{NOUN[kind]} tables"
    want0, want1 = w.direct(kind, (0,)), w.direct(kind, (1,))

    def both_as_before(a, b, b_want=want1):
        assert finished(kind, a) == want0 and finished(kind, b) == b_want

    # with itself
    with w.table(kind, 0, [0]) as a:
        refused(w, lambda: a.absorb(a), ARG, f"{fn}: bad argument")
        assert finished(kind, a) == want0
    # through another context than the destination's
    with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1]) as b:
        with through(a, w.ctx[1]):
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: the table to merge into belongs to another context")
        both_as_before(a, b)
    # into and from a finished table
    with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1]) as b:
        assert finished(kind, a) == want0
        refused(w, lambda: a.absorb(b), ARG, f"{fn}: one of the {tables} is finished")
        refused(w, lambda: b.absorb(a), ARG, f"{fn}: one of the {tables} is finished")
        both_as_before(a, b)
    # the same page (batch tables) or the same (page, identifier) (run tables) in both
    with w.table(kind, 0, [0]) as a, w.table(kind, 1, [0, 1]) as b:
        overlap = f"page 0 is merged into both {tables}" if kind in BATCH else f"a query identifier is merged for page 0 into both {tables}"
        refused(w, lambda: a.absorb(b), ARG, f"{fn}: {overlap}")
        both_as_before(a, b, w.direct(kind, (0, 1)))
    # distinct_sites 0 and 1
    with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1], distinct=1) as b:
        refused(w, lambda: a.absorb(b), ARG, f"{fn}: the {tables} hold pages searched with distinct_sites 0 and 1")
        refused(w, lambda: b.absorb(a), ARG, f"{fn}: the {tables} hold pages searched with distinct_sites 1 and 0")
        both_as_before(a, b, w.direct(kind, (1,), distinct=1))
    if kind in ("top", "tophits", "targets"):
        per = "target" if kind == "targets" else "query"
        # another n
        with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1], n=N + 1) as b:
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: the {tables} keep {N} and {N + 1} records per {per}")
            refused(w, lambda: b.absorb(a), ARG, f"{fn}: the {tables} keep {N + 1} and {N} records per {per}")
            both_as_before(a, b, w.direct(kind, (1,), n=N + 1))
        # another n and a finished source: the finished table is what the call reports
        with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1], n=N + 1) as b:
            assert finished(kind, b) == w.direct(kind, (1,), n=N + 1)
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: one of the {tables} is finished")
            both_as_before(a, b, w.direct(kind, (1,), n=N + 1))
    if kind == "tophits":
        with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1], style=0) as b:
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: the {tables} hold pages searched with output_style 1 and 0")
            both_as_before(a, b, w.direct(kind, (1,), style=0))
        # ... which is asked before anything else: a finished source of another style
        with w.table(kind, 0, [0]) as a, w.table(kind, 1, [1], style=0) as b:
            assert finished(kind, b) == w.direct(kind, (1,), style=0)
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: the {tables} hold pages searched with output_style 1 and 0")
            both_as_before(a, b, w.direct(kind, (1,), style=0))
    if kind in RUN:
        # databases of different shape
        with w.table(kind, 0, [0]) as a, w.empty(kind, 1, db=w.small) as b:
            refused(w, lambda: a.absorb(b), ARG, f"{fn}: the {tables} were made for different databases")
            refused(w, lambda: b.absorb(a), ARG, f"{fn}: the {tables} were made for different databases")
            assert finished(kind, a) == want0
            arrays, counts = finished(kind, b)
            assert counts == (0, 0, 0) and not any(arrays)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_page_merges(world, kind):
    w = world
    fn, table = f"prb_search_page_{kind}", f"{NOUN[kind]} table"
    want0 = w.direct(kind, (0,))
    # merged twice
    with w.table(kind, 0, [0]) as t:
        twice = f"page 0 is already merged into this {table}" if kind in BATCH else "query identifier 0 is already merged for page 0"
        refused(w, lambda: w.add(kind, t, 0, 0), ARG, f"{fn}: {twice}")
        if kind in RUN:
            refused(w, lambda: w.add(kind, t, 0, 0, ids=(7, 2, 9)), ARG, f"{fn}: query identifier 2 is already merged for page 0")
            # identifiers below 0 and given twice: none of the call's identifiers counts as merged afterwards
            refused(w, lambda: w.add(kind, t, 0, 1, ids=(4, -1, 5)), ARG, f"{fn}: query identifier -1 is below 0")
            refused(w, lambda: w.add(kind, t, 0, 1, ids=(5, 3, 5)), ARG, f"{fn}: query identifier 5 is given twice")
        # distinct_sites 0, then 1
        refused(w, lambda: w.add(kind, t, 0, 1, distinct=1), ARG,
                f"{fn}: the {table} holds pages searched with distinct_sites 0 (this call: 1)")
        if kind == "tophits":
            refused(w, lambda: w.add(kind, t, 0, 1, style=0), ARG,
                    f"{fn}: the {table} holds pages searched with output_style 1 (this call: 0)")
        # through another context
        with through(t, w.ctx[1]):
            other = (f"the {table} was made for another context or query batch (3 queries; this batch has 3)" if kind in BATCH else
                     f"the {table} was made with another context or for another database")
            refused(w, lambda: w.add(kind, t, 1, 1), ARG, f"{fn}: {other}")
        assert finished(kind, t) == want0
        # into a finished table
        refused(w, lambda: w.add(kind, t, 0, 1), STATE, f"{fn}: the {table} is finished (prb_{PREFIX[kind]}_finish)")
        assert finished(kind, t) == want0
    # every refusal above left page 1 and its identifiers free
    with w.table(kind, 0, [0]) as t:
        if kind in RUN:
            refused(w, lambda: w.add(kind, t, 0, 1, ids=(4, -1, 5)), ARG, f"{fn}: query identifier -1 is below 0")
            refused(w, lambda: w.add(kind, t, 0, 1, ids=(5, 3, 5)), ARG, f"{fn}: query identifier 5 is given twice")
        refused(w, lambda: w.add(kind, t, 0, 1, distinct=1), ARG,
                f"{fn}: the {table} holds pages searched with distinct_sites 0 (this call: 1)")
        w.add(kind, t, 0, 1)
        assert finished(kind, t) == w.direct(kind, (0, 1))


@pytest.mark.parametrize("kind", KINDS)
def test_finish_guards(world, kind):
    w, fn = world, f"prb_{PREFIX[kind]}_finish"
    want0 = w.direct(kind, (0,))
    with w.table(kind, 0, [0]) as t:
        with through(t, w.ctx[1]):
            refused(w, lambda: finished(kind, t), ARG, f"{fn}: bad argument (the table belongs to another context)")
        first = finished(kind, t)
        assert first == want0
        # a second finish is no error and gives the same records, whatever was refused in between
        assert finished(kind, t) == first
        with through(t, w.ctx[1]):
            refused(w, lambda: finished(kind, t), ARG, f"{fn}: bad argument (the table belongs to another context)")
        assert finished(kind, t) == first
