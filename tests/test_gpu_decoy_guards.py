"""GPU tests of what the four tables around the decoys refuse (prb_nullset_*, prb_groupset_*, prb_gnullset_*,
prb_evalset_* and their prb_search_page_* entry points): the error code and the whole error text of every refused call,
which refusal wins where a call breaks two conditions at once, and that a refused call leaves its table as it was - it
still finishes to the bytes it gives without the call.  The texts are spelled out here; what the tables hold is pinned by
test_gpu_null*.py, test_gpu_group*.py, test_gpu_gnull*.py and test_gpu_eval*.py.

Shapes: the c1 golden targets (32) as two pages of 16, two of the c1 queries, 3 decoys per query, one context on device
0.  The lists are hand-made (page 0's real records: one search of the page, shared); of the search entry points only
what they refuse is asked, which costs no search, after one page of the real batch is in - one search of 16 targets per
table.  The evalset takes a second one, of two decoys: nothing but a search marks its (page, query, decoy) as merged.
The device's `bad` flag is reached through prb_evalset_add_keys alone: every other list is checked whole on the host."""
import os

import numpy as np
import pytest

import refdump

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARG, STATE = -1, -5
NQ, ND, NSEQ = 2, 3, 16
ALL = [(q, d) for q in range(NQ) for d in range(ND)]
OWNER, DECOY = [q for q, _ in ALL], [d for _, d in ALL]
MAPS, NG = [[i // 4 for i in range(NSEQ)], [4 + i // 4 for i in range(NSEQ)]], 8
MASK_WHY = "allowed_pairs was made for another query batch, another database or on another device"
EVAL_BAD = ("a record merged into this evalset named a query, an owner or a decoy outside it, or a key was looked up that it "
            "does not hold")


def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records with every other field filled in recognisably"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + i % 3, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


class World:
    """one context, the database, the real batch, two batches of its decoys (all six; the last two), page 0's records"""

    def __init__(self, tmp):
        from priblast_amd import capi
        self.capi = capi
        names, targets = refdump.read_fasta(os.path.join(GOLDEN, "c1_db.fa"))
        _, queries = refdump.read_fasta(os.path.join(GOLDEN, "c1_q.fa"))
        self.ctx = capi.Context(0)
        capi.db_build(self.ctx, str(tmp / "c1"), names, targets, page_size=NSEQ)
        self.db = capi.Db(self.ctx, str(tmp / "c1"))
        assert self.db.npages == 2
        dseqs, owner, decoy = capi.null_decoys(queries[:NQ], ND)
        assert list(owner) == OWNER and list(decoy) == DECOY
        self.qb, self.dqb6, self.dqb2 = (capi.QBatch(self.ctx, s, self.db.repeat_flag) for s in (queries[:NQ], dseqs, dseqs[4:]))
        for b in (self.qb, self.dqb6, self.dqb2):
            b.accessibility(self.db.W, self.db.delta)
        self.mask_real, self.mask_decoys = capi.PairMask(self.ctx, self.qb, self.db), capi.PairMask(self.ctx, self.dqb6, self.db)
        # the real batch: page 0 as the search gives it, page 1 by hand
        self.real = {0: capi.search_page_summary(self.ctx, self.qb, self.db, 0), 1: pairs([(0, 1, -9.0), (1, 15, -8.0)])}
        assert len(self.real[0]) and set(self.real[0]["query"]) == {0, 1}
        self.hits0 = capi.search_page(self.ctx, self.qb, self.db, 0)[0]

    def close(self):
        for x in (self.mask_real, self.mask_decoys, self.dqb2, self.dqb6, self.qb, self.db, self.ctx):
            x.close()

    def opts(self, distinct=0, mask=None):
        o = self.capi.default_opts(distinct_sites=distinct)
        if mask is not None:
            o.allowed_pairs = mask.h.value
        return o

    def decoy_records(self, batch, page):
        """the records of the batch's decoys against the page: `query` = the decoy's place in the batch.  Decoy d of query q
        reaches q's first observed pair of page 0 at -100 - d, and some target of page 1 at -1"""
        first = {q: int(self.real[0]["db_id"][self.real[0]["query"] == q][0]) for q in range(NQ)}
        if page == 0:
            return pairs([(k, first[q], -100.0 - d) for k, (q, d) in enumerate(batch)])
        return pairs([(k, (1, 15)[q] if d else 7, -1.0) for k, (q, d) in enumerate(batch)])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("decoyguards"))
    yield w
    w.close()


def refused(w, call, code, text):
    with pytest.raises(w.capi.PrbError) as err:
        call()
    assert str(err.value) == f"libpriblast_hip error {code}: {text}"


# ---- the null table

def null_table(w, searched, refusals):
    """page 0 by a search or from the list, page 1 from the list, every decoy from lists -> the finished bytes"""
    with w.capi.NullSet(w.ctx, w.qb, w.db, ND) as ns:
        if searched:
            ns.observed(0, w.opts())
        else:
            ns.observe(0, w.real[0])
        if refusals:
            null_refusals_before_page_1(w, ns, searched)
        ns.observe(1, w.real[1])
        ns.add_pairs(0, OWNER, DECOY, w.decoy_records(ALL, 0))
        if refusals:
            null_refusals_after_page_0(w, ns)
        ns.add_pairs(1, OWNER[:2], DECOY[:2], w.decoy_records(ALL[:2], 1))
        if refusals:
            refused(w, ns.finish, STATE, "prb_nullset_finish: 8 of 12 (query, decoy, page) searches are merged: every decoy of every query "
                    "against every page comes first")
        ns.add_pairs(1, OWNER[2:], DECOY[2:], w.decoy_records(ALL[2:], 1))
        return ns.finish().tobytes()


def null_refusals_before_page_1(w, ns, searched):
    fn, good = "prb_nullset_add_pairs", w.decoy_records(ALL, 0)
    refused(w, lambda: ns.add_pairs(1, [0], [0], pairs([])), STATE,
            f"{fn}: page 1 is not observed yet (the real batch's search comes first)")
    refused(w, lambda: ns.decoys(w.dqb6, 1, OWNER, DECOY, w.opts()), STATE,
            "prb_search_page_decoys: page 1 is not observed yet (the real batch's search comes first)")
    refused(w, lambda: ns.observe(0, w.real[0]), ARG, "prb_nullset_observe: page 0 is already observed in this null table")
    refused(w, lambda: ns.observe(2, pairs([])), ARG, "prb_nullset_observe: page 2 out of range (the database has 2)")
    refused(w, lambda: ns.observe(1, pairs([(NQ, 0, -9.0)])), ARG,
            "prb_nullset_observe: pair record 0 is out of range (query 2 of 2, db_id 0 of 16, hits 1)")
    refused(w, lambda: ns.observe(1, pairs([(1, 3, -9.0), (0, 3, -9.0), (1, 3, -8.0)])), ARG,
            "prb_nullset_observe: the pair (query 1, db_id 3) has two records")
    # the decoys' owners and numbers
    refused(w, lambda: ns.add_pairs(0, [0, NQ], [0, 0], pairs([])), ARG, f"{fn}: owner[1] = 2 is out of range (the batch has 2 queries)")
    refused(w, lambda: ns.add_pairs(0, [-1], [0], pairs([])), ARG, f"{fn}: owner[0] = -1 is out of range (the batch has 2 queries)")
    refused(w, lambda: ns.add_pairs(0, [0], [ND], pairs([])), ARG, f"{fn}: decoy[0] = 3 is out of range (the table has 3 decoys per query)")
    refused(w, lambda: ns.add_pairs(0, [0], [-1], pairs([])), ARG, f"{fn}: decoy[0] = -1 is out of range (the table has 3 decoys per query)")
    refused(w, lambda: ns.add_pairs(0, [1, 0, 1], [0, 2, 0], pairs([])), ARG, f"{fn}: decoy 0 of query 1 is given twice")
    # ... an owner out of range behind a pair given twice: the ranges are asked first
    refused(w, lambda: ns.add_pairs(0, [1, 1, 5], [0, 0, 0], pairs([])), ARG, f"{fn}: owner[2] = 5 is out of range (the batch has 2 queries)")
    # the records: `query` indexes the call's owners
    refused(w, lambda: ns.add_pairs(0, [0], [0], pairs([(1, 0, -9.0)])), ARG,
            f"{fn}: pair record 0 is out of range (query 1 of 1, db_id 0 of 16, hits 1)")
    refused(w, lambda: ns.add_pairs(0, [0], [0], pairs([(0, 0, -9.0), (0, NSEQ, -9.0)])), ARG,
            f"{fn}: pair record 1 is out of range (query 0 of 1, db_id 16 of 16, hits 2)")
    no_hit = good.copy()
    no_hit["hits"][2] = 0
    refused(w, lambda: ns.add_pairs(0, OWNER, DECOY, no_hit), ARG,
            f"{fn}: pair record 2 is out of range (query 2 of 6, db_id {no_hit['db_id'][2]} of 16, hits 0)")
    refused(w, lambda: ns.add_pairs(0, [0], [0], pairs([(0, 3, -9.0), (0, 3, -8.0)])), ARG, f"{fn}: the pair (query 0, db_id 3) has two records")
    # ... a page out of range wins over the owners, the owners over the records
    refused(w, lambda: ns.add_pairs(2, [NQ], [0], pairs([])), ARG, f"{fn}: page 2 out of range (the database has 2)")
    refused(w, lambda: ns.add_pairs(-1, [0], [0], pairs([])), ARG, f"{fn}: page -1 out of range (the database has 2)")
    refused(w, lambda: ns.add_pairs(0, [0], [ND], pairs([(1, 0, -9.0)])), ARG,
            f"{fn}: decoy[0] = 3 is out of range (the table has 3 decoys per query)")
    if searched:
        fn = "prb_search_page_observed"
        clash = "the null table holds pages searched with distinct_sites 0 (this call: 1)"
        refused(w, lambda: ns.observed(0, w.opts()), ARG, f"{fn}: page 0 is already observed in this null table")
        refused(w, lambda: ns.observed(2, w.opts()), ARG, f"{fn}: bad argument")
        refused(w, lambda: ns.observed(1, w.opts(mask=w.mask_decoys)), ARG, f"{fn}: {MASK_WHY}")
        refused(w, lambda: ns.observed(1, w.opts(distinct=1)), ARG, f"{fn}: {clash}")
        # ... the selection is asked before the mask, the mask before the page
        refused(w, lambda: ns.observed(1, w.opts(distinct=1, mask=w.mask_decoys)), ARG, f"{fn}: {clash}")
        refused(w, lambda: ns.observed(0, w.opts(mask=w.mask_decoys)), ARG, f"{fn}: {MASK_WHY}")
        fn = "prb_search_page_decoys"
        refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, DECOY, w.opts(mask=w.mask_real)), ARG, f"{fn}: {MASK_WHY}")
        refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, DECOY, w.opts(distinct=1)), ARG, f"{fn}: {clash}")
        refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, DECOY, w.opts(distinct=1, mask=w.mask_real)), ARG, f"{fn}: {clash}")
        refused(w, lambda: ns.decoys(w.dqb6, 2, OWNER, DECOY, w.opts()), ARG, f"{fn}: bad argument")
        bad_owner = [NQ] + OWNER[1:]
        refused(w, lambda: ns.decoys(w.dqb6, 0, bad_owner, DECOY, w.opts()), ARG, f"{fn}: owner[0] = 2 is out of range (the batch has 2 queries)")
        refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, [ND] + DECOY[1:], w.opts()), ARG,
                f"{fn}: decoy[0] = 3 is out of range (the table has 3 decoys per query)")
        refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, [0, 1, 1, 0, 1, 2], w.opts()), ARG, f"{fn}: decoy 1 of query 0 is given twice")
        # ... the mask is asked before the owners
        refused(w, lambda: ns.decoys(w.dqb6, 0, bad_owner, DECOY, w.opts(mask=w.mask_real)), ARG, f"{fn}: {MASK_WHY}")
    refused(w, ns.finish, STATE, "prb_nullset_finish: 0 of 12 (query, decoy, page) searches are merged: every decoy of every query against "
            "every page comes first")


def null_refusals_after_page_0(w, ns):
    fn = "prb_nullset_add_pairs"
    refused(w, lambda: ns.add_pairs(0, [1], [2], pairs([])), ARG, f"{fn}: decoy 2 of query 1 is already merged for page 0")
    # ... which is asked decoy by decoy with the ranges, and before a pair given twice
    refused(w, lambda: ns.add_pairs(0, [0, NQ], [1, 0], pairs([])), ARG, f"{fn}: decoy 1 of query 0 is already merged for page 0")
    refused(w, lambda: ns.add_pairs(0, [NQ, 0], [0, 1], pairs([])), ARG, f"{fn}: owner[0] = 2 is out of range (the batch has 2 queries)")
    refused(w, lambda: ns.add_pairs(0, [0, 0], [1, 1], pairs([])), ARG, f"{fn}: decoy 1 of query 0 is already merged for page 0")
    refused(w, lambda: ns.decoys(w.dqb6, 0, OWNER, DECOY, w.opts()), ARG,
            "prb_search_page_decoys: decoy 0 of query 0 is already merged for page 0")
    # page 1 took none of it
    refused(w, ns.finish, STATE, "prb_nullset_finish: 6 of 12 (query, decoy, page) searches are merged: every decoy of every query against "
            "every page comes first")


def test_null_table(world):
    w = world
    want = null_table(w, False, False)
    assert len(want) == (len(w.real[0]) + len(w.real[1])) * w.capi.NULL_DTYPE.itemsize
    assert null_table(w, False, True) == want
    assert null_table(w, True, True) == want


# ---- the group table

def group_table(w, searched, refusals, finish=True):
    """page 0 by a search or from the list, page 1 from the list -> the table and - finish - its bytes"""
    gs = w.capi.GroupSet(w.ctx, w.qb, w.db, MAPS, NG)
    fn = "prb_groupset_add_pairs"
    if refusals:
        refused(w, lambda: gs.add_pairs(2, pairs([])), ARG, f"{fn}: page 2 out of range (the database has 2)")
        refused(w, lambda: gs.add_pairs(-1, pairs([])), ARG, f"{fn}: page -1 out of range (the database has 2)")
    if searched:
        gs.merge(0, w.opts())
    else:
        gs.add_pairs(0, w.real[0])
    if refusals:
        refused(w, lambda: gs.add_pairs(0, w.real[0]), ARG, f"{fn}: page 0 is already merged into this group table")
        refused(w, lambda: gs.add_pairs(1, pairs([(0, 0, -9.0), (NQ, 0, -9.0)])), ARG,
                f"{fn}: pair record 1 is out of range (query 2 of 2, db_id 0 of 16, hits 2)")
        refused(w, lambda: gs.add_pairs(1, pairs([(0, -1, -9.0)])), ARG, f"{fn}: pair record 0 is out of range (query 0 of 2, db_id -1 of 16, hits 1)")
        refused(w, lambda: gs.add_pairs(1, pairs([(1, 3, -9.0), (0, 3, -9.0), (1, 3, -8.0)])), ARG, f"{fn}: the pair (query 1, db_id 3) has two records")
        # ... the page is asked before the records
        refused(w, lambda: gs.add_pairs(0, pairs([(NQ, 0, -9.0)])), ARG, f"{fn}: page 0 is already merged into this group table")
        refused(w, lambda: gs.add_pairs(2, pairs([(NQ, 0, -9.0)])), ARG, f"{fn}: page 2 out of range (the database has 2)")
        refused(w, lambda: gs.finish(1025), ARG, "prb_groupset_finish: need 0 <= n <= 1024 (got 1025)")
        refused(w, lambda: w.capi.GNullSet(w.ctx, gs, 0, ND), STATE,
                "prb_gnullset_create: page 1 is not merged into the group table: the real batch against every page comes first")
        refused(w, lambda: w.capi.GNullSet(w.ctx, gs, 0, 0), ARG, "prb_gnullset_create: need 1 <= ndecoys <= 100000 (got 0)")
    if refusals and searched:
        fn = "prb_search_page_groups"
        refused(w, lambda: gs.merge(0, w.opts()), ARG, f"{fn}: page 0 is already merged into this group table")
        refused(w, lambda: gs.merge(1, w.opts(distinct=1)), ARG, f"{fn}: the group table holds pages searched with distinct_sites 0 (this call: 1)")
        refused(w, lambda: gs.merge(2, w.opts()), ARG, f"{fn}: bad argument")
    gs.add_pairs(1, w.real[1])
    if not finish:
        return gs
    with gs:
        got = gs.finish().tobytes()
        if refusals:
            refused(w, lambda: gs.add_pairs(1, w.real[1]), STATE, "prb_groupset_add_pairs: the group table is finished (prb_groupset_finish)")
            assert gs.finish().tobytes() == got
        return got


def test_group_table(world):
    w = world
    want = group_table(w, False, False)
    assert len(want) >= 2 * w.capi.GROUP_DTYPE.itemsize
    assert group_table(w, False, True) == want
    assert group_table(w, True, True) == want


# ---- the group null table

def add_batch(w, gn, batch):
    gn.begin([q for q, _ in batch], [d for _, d in batch])
    for p in (0, 1):
        gn.add_pairs(p, w.decoy_records(batch, p))
    gn.end()


def gnull_table(w, searched, refusals):
    """the group table above into a group null table, the decoys as batches of four and two from lists -> the bytes"""
    first, second = ALL[:4], ALL[4:]
    begin, add, end, fin = (f"prb_gnullset_{x}" for x in ("begin", "add_pairs", "end", "finish"))
    merge = "prb_search_page_gnull"
    is_open = "a decoy batch is open (prb_gnullset_end comes first)"
    with group_table(w, searched, refusals, finish=False) as gs, w.capi.GNullSet(w.ctx, gs, 0, ND) as gn:
        if not refusals:
            add_batch(w, gn, first)
            add_batch(w, gn, second)
            return gn.finish().tobytes()
        refused(w, lambda: gn.add_pairs(0, pairs([])), STATE, f"{add}: no decoy batch is open (prb_gnullset_begin comes first)")
        refused(w, lambda: gn.merge(w.dqb6, 0, w.opts()), STATE, f"{merge}: no decoy batch is open (prb_gnullset_begin comes first)")
        refused(w, gn.end, STATE, f"{end}: no decoy batch is open")
        refused(w, lambda: gn.begin([], []), ARG, f"{begin}: bad argument (a batch has one decoy at least)")
        refused(w, lambda: gn.begin([0, NQ], [0, 0]), ARG, f"{begin}: owner[1] = 2 is out of range (the batch has 2 queries)")
        refused(w, lambda: gn.begin([-1], [0]), ARG, f"{begin}: owner[0] = -1 is out of range (the batch has 2 queries)")
        refused(w, lambda: gn.begin([0], [ND]), ARG, f"{begin}: decoy[0] = 3 is out of range (the table has 3 decoys per query)")
        refused(w, lambda: gn.begin([0, 1, 0], [1, 1, 1]), ARG, f"{begin}: decoy 1 of query 0 is given twice")
        # ... an owner out of range behind a pair given twice: the ranges are asked first
        refused(w, lambda: gn.begin([1, 1, 5], [0, 0, 0]), ARG, f"{begin}: owner[2] = 5 is out of range (the batch has 2 queries)")
        refused(w, gn.finish, STATE, f"{fin}: 0 of 6 (query, decoy) pairs are closed: every decoy of every query comes first")
        gn.begin([q for q, _ in first], [d for _, d in first])
        # ... an open batch wins over the owners
        refused(w, lambda: gn.begin([NQ], [0]), STATE, f"{begin}: {is_open}")
        refused(w, gn.finish, STATE, f"{fin}: {is_open}")
        refused(w, lambda: gn.add_pairs(2, pairs([])), ARG, f"{add}: page 2 out of range (the database has 2)")
        refused(w, lambda: gn.add_pairs(0, pairs([(4, 0, -9.0)])), ARG, f"{add}: pair record 0 is out of range (query 4 of 4, db_id 0 of 16, hits 1)")
        refused(w, lambda: gn.add_pairs(0, pairs([(0, 0, -9.0), (3, NSEQ, -9.0)])), ARG,
                f"{add}: pair record 1 is out of range (query 3 of 4, db_id 16 of 16, hits 2)")
        refused(w, lambda: gn.add_pairs(0, pairs([(0, 3, -9.0), (0, 3, -8.0)])), ARG, f"{add}: the pair (query 0, db_id 3) has two records")
        gn.add_pairs(0, w.decoy_records(first, 0))
        refused(w, lambda: gn.add_pairs(0, w.decoy_records(first, 0)), ARG, f"{add}: page 0 is already merged in the open decoy batch")
        # ... the page is asked before the records
        refused(w, lambda: gn.add_pairs(0, pairs([(4, 0, -9.0)])), ARG, f"{add}: page 0 is already merged in the open decoy batch")
        refused(w, gn.end, STATE, f"{end}: page 1 is not merged in the open decoy batch: every page comes first")
        gn.add_pairs(1, w.decoy_records(first, 1))
        gn.end()
        refused(w, lambda: gn.begin([1, 0], [1, 0]), ARG, f"{begin}: decoy 0 of query 0 belongs to a batch closed before")
        # ... which is asked decoy by decoy with the ranges, and before a pair given twice
        refused(w, lambda: gn.begin([0, NQ], [1, 0]), ARG, f"{begin}: decoy 1 of query 0 belongs to a batch closed before")
        refused(w, lambda: gn.begin([NQ, 0], [0, 1]), ARG, f"{begin}: owner[0] = 2 is out of range (the batch has 2 queries)")
        refused(w, lambda: gn.begin([0, 0], [1, 1]), ARG, f"{begin}: decoy 1 of query 0 belongs to a batch closed before")
        refused(w, gn.finish, STATE, f"{fin}: 4 of 6 (query, decoy) pairs are closed: every decoy of every query comes first")
        gn.begin([q for q, _ in second], [d for _, d in second])
        # the search of a page into the open batch of two
        refused(w, lambda: gn.merge(w.dqb6, 0, w.opts()), ARG, f"{merge}: the open decoy batch has 2 decoys; this query batch has 6")
        refused(w, lambda: gn.merge(w.dqb2, 2, w.opts()), ARG, f"{merge}: bad argument")
        refused(w, lambda: gn.merge(w.dqb2, 0, w.opts(mask=w.mask_real)), ARG, f"{merge}: {MASK_WHY}")
        if searched:  # (a group table made from lists alone holds no selection)
            clash = "the group null table holds pages searched with distinct_sites 0 (this call: 1)"
            refused(w, lambda: gn.merge(w.dqb2, 0, w.opts(distinct=1)), ARG, f"{merge}: {clash}")
            # ... the batch's size is asked before the selection, the selection before the mask
            refused(w, lambda: gn.merge(w.dqb6, 0, w.opts(distinct=1)), ARG, f"{merge}: the open decoy batch has 2 decoys; this query batch has 6")
            refused(w, lambda: gn.merge(w.dqb2, 0, w.opts(distinct=1, mask=w.mask_real)), ARG, f"{merge}: {clash}")
        for p in (0, 1):
            gn.add_pairs(p, w.decoy_records(second, p))
        refused(w, lambda: gn.merge(w.dqb2, 1, w.opts()), ARG, f"{merge}: page 1 is already merged in the open decoy batch")
        gn.end()
        got = gn.finish().tobytes()
        assert gn.finish().tobytes() == got
        refused(w, lambda: gn.begin([0], [0]), STATE, f"{begin}: the group null table is finished (prb_gnullset_finish)")
        return got


def test_group_null_table(world):
    w = world
    want = gnull_table(w, False, False)
    assert len(want) >= 2 * w.capi.GNULL_DTYPE.itemsize
    assert gnull_table(w, False, True) == want
    assert gnull_table(w, True, True) == want


# ---- the evalset

def eval_lists(w, refusals):
    """the keys of page 0's hits as the real list, one decoy key per (query, decoy) -> the scores' bytes"""
    q, e = w.hits0["query"], w.hits0["e_tot"]
    fn = "prb_search_page_null_hits"
    with w.capi.EvalSet(w.ctx, w.qb, w.db, ND) as es:
        es.add_keys(0, q, e)
        if refusals:
            refused(w, lambda: es.null_hits(w.dqb6, 0, [NQ] + OWNER[1:], DECOY, w.opts()), ARG,
                    f"{fn}: owner[0] = 2 is out of range (the batch has 2 queries)")
            refused(w, lambda: es.null_hits(w.dqb6, 0, OWNER[:5] + [-1], DECOY, w.opts()), ARG,
                    f"{fn}: owner[5] = -1 is out of range (the batch has 2 queries)")
            refused(w, lambda: es.null_hits(w.dqb6, 0, OWNER, [ND] + DECOY[1:], w.opts()), ARG,
                    f"{fn}: decoy[0] = 3 is out of range (the table has 3 decoys per query)")
            refused(w, lambda: es.null_hits(w.dqb6, 1, OWNER, [0, 1, 1, 0, 1, 2], w.opts()), ARG, f"{fn}: decoy 1 of query 0 is given twice")
            # ... an owner out of range behind a pair given twice: the ranges are asked first
            refused(w, lambda: es.null_hits(w.dqb6, 1, [0, 0, 0, 1, 1, 5], [0, 0, 1, 0, 1, 2], w.opts()), ARG,
                    f"{fn}: owner[5] = 5 is out of range (the batch has 2 queries)")
            refused(w, lambda: es.null_hits(w.dqb6, 2, OWNER, DECOY, w.opts()), ARG, f"{fn}: bad argument")
            refused(w, lambda: es.null_hits(w.dqb6, 0, OWNER, DECOY, w.opts(mask=w.mask_real)), ARG, f"{fn}: {MASK_WHY}")
            # ... the mask is asked before the owners
            refused(w, lambda: es.null_hits(w.dqb6, 0, [NQ] + OWNER[1:], DECOY, w.opts(mask=w.mask_real)), ARG, f"{fn}: {MASK_WHY}")
            refused(w, lambda: es.scored(1, w.opts(mask=w.mask_decoys)), ARG, f"prb_search_page_scored: {MASK_WHY}")
            refused(w, lambda: es.scored(2, w.opts()), ARG, "prb_search_page_scored: bad argument")
            refused(w, lambda: es.score(q[:1], e[:1]), STATE, "prb_evalset_score: the evalset is not closed yet (prb_evalset_close)")
            assert es.sizes() == (len(q), 0)
        es.add_keys(1, OWNER, [float(np.min(e)) + 0.5 * d for d in DECOY])
        es.finish()
        got = es.score(q, e).tobytes()
        if refusals:
            es.finish()  # (a second close does nothing)
            refused(w, lambda: es.add_keys(0, q, e), STATE, "prb_evalset_add_keys: the evalset is closed (prb_evalset_close)")
            refused(w, lambda: es.null_hits(w.dqb6, 0, OWNER, DECOY, w.opts()), STATE, f"{fn}: the evalset is closed (prb_evalset_close)")
            assert es.score(q, e).tobytes() == got
        return got


def test_evalset_lists(world):
    w = world
    want = eval_lists(w, False)
    assert len(want) == len(w.hits0) * w.capi.EVAL_DTYPE.itemsize and len(w.hits0)
    assert eval_lists(w, True) == want


def test_evalset_searches(world):
    """one page of the real batch and two decoys against it searched; everything behind is refused and leaves the lists"""
    w = world
    scored, hits, close = "prb_search_page_scored", "prb_search_page_null_hits", "prb_evalset_close"
    clash = "the evalset holds pages searched with distinct_sites 0 (this call: 1)"
    missing = ("(query, decoy, page) searches are merged: every page, and every decoy of every query against every page, comes first")
    with w.capi.EvalSet(w.ctx, w.qb, w.db, ND) as es:
        es.scored(0, w.opts())
        sizes, counts = es.sizes(), es.counts()
        assert sizes == (len(w.hits0), 0) and counts[2] == len(w.hits0)
        refused(w, lambda: es.scored(0, w.opts()), ARG, f"{scored}: page 0 is already merged into this evalset")
        refused(w, lambda: es.scored(1, w.opts(distinct=1)), ARG, f"{scored}: {clash}")
        refused(w, lambda: es.scored(1, w.opts(mask=w.mask_decoys)), ARG, f"{scored}: {MASK_WHY}")
        # ... the selection is asked before the mask, the mask before the page
        refused(w, lambda: es.scored(1, w.opts(distinct=1, mask=w.mask_decoys)), ARG, f"{scored}: {clash}")
        refused(w, lambda: es.scored(0, w.opts(mask=w.mask_decoys)), ARG, f"{scored}: {MASK_WHY}")
        refused(w, lambda: es.null_hits(w.dqb2, 0, [1, 1], [1, 2], w.opts(distinct=1)), ARG, f"{hits}: {clash}")
        refused(w, lambda: es.null_hits(w.dqb2, 0, [1, 1], [1, 2], w.opts(distinct=1, mask=w.mask_real)), ARG, f"{hits}: {clash}")
        refused(w, es.finish, STATE, f"{close}: 1 of 2 pages of the real batch and 0 of 12 {missing}")
        assert es.sizes() == sizes and es.counts() == counts and es.decoy_counts() == (0, 0, 0)
        es.null_hits(w.dqb2, 0, [1, 1], [1, 2], w.opts())
        sizes, dcounts = es.sizes(), es.decoy_counts()
        assert sizes[0] == len(w.hits0) and sizes[1] == dcounts[2]
        refused(w, lambda: es.null_hits(w.dqb2, 0, [1, 1], [1, 2], w.opts()), ARG, f"{hits}: decoy 1 of query 1 is already merged for page 0")
        # ... which is asked decoy by decoy with the ranges, and before a pair given twice
        refused(w, lambda: es.null_hits(w.dqb2, 0, [1, NQ], [2, 0], w.opts()), ARG, f"{hits}: decoy 2 of query 1 is already merged for page 0")
        refused(w, lambda: es.null_hits(w.dqb2, 0, [NQ, 1], [0, 2], w.opts()), ARG, f"{hits}: owner[0] = 2 is out of range (the batch has 2 queries)")
        refused(w, lambda: es.null_hits(w.dqb2, 0, [1, 1], [2, 2], w.opts()), ARG, f"{hits}: decoy 2 of query 1 is already merged for page 0")
        refused(w, lambda: es.null_hits(w.dqb2, 1, [1, 1], [2, 2], w.opts()), ARG, f"{hits}: decoy 2 of query 1 is given twice")
        refused(w, es.finish, STATE, f"{close}: 1 of 2 pages of the real batch and 2 of 12 {missing}")
        assert es.sizes() == sizes and es.counts() == counts and es.decoy_counts() == dcounts


def test_evalset_device_flag(world):
    """an owner outside the table: the kernel raises the flag and writes nothing, the call returns, every later one is refused"""
    w = world
    for is_decoy, ids in ((1, [0, NQ]), (0, [-1])):
        with w.capi.EvalSet(w.ctx, w.qb, w.db, ND) as es:
            es.add_keys(0, [0], [-9.0])
            es.add_keys(is_decoy, ids, [-9.0] * len(ids))
            refused(w, lambda: es.add_keys(0, [0], [-8.0]), STATE, f"prb_evalset_add_keys: {EVAL_BAD}")
            refused(w, lambda: es.null_hits(w.dqb6, 0, OWNER, DECOY, w.opts()), STATE, f"prb_search_page_null_hits: {EVAL_BAD}")
            refused(w, es.finish, STATE, f"prb_evalset_close: {EVAL_BAD}")
