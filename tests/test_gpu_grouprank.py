"""GPU tests of the group ranking table on the search path (prb_search_page_groups into a group table, then
prb_grouprank_add_groupset) through the C ABI, on the `mix` fixture - 3 pages, four consecutive targets to a group, so
groups span the pages' borders - and on the `edge` fixture (tiny, adjacent and page-edge targets in 5 pages).  The
yardstick is tests/grouprank_ref.py's restatement, fed with the group table's own records (prb_groupset_finish(gs, 0),
pinned by test_gpu_group.py): the table must match it byte for byte, however the queries are cut into batches."""
import os

import numpy as np
import pytest

import grouprank_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def group_maps(db, per_group):
    """consecutive targets of the whole database, `per_group` to a group (so groups span the pages' borders)"""
    maps, t = [], 0
    for p in range(db.npages):
        nseq = db.page_info(p)[0]
        maps.append([(t + i) // per_group for i in range(nseq)])
        t += nseq
    return maps, (t + per_group - 1) // per_group


class Case:
    """a database, its queries under identifiers of the caller's, and per cut of the queries into batches the QBatches"""

    def __init__(self, ctx, prefix, seqs, per_group):
        from priblast_amd import capi
        self.ctx, self.seqs = ctx, seqs
        self.db = capi.Db(ctx, prefix)
        self.maps, self.ng = group_maps(self.db, per_group)
        self.ids = [5 * q + 2 for q in range(len(seqs))][::-1]
        self.batches = {}

    def batch(self, qs):
        from priblast_amd import capi
        if qs not in self.batches:
            qb = capi.QBatch(self.ctx, [self.seqs[q] for q in qs], self.db.repeat_flag)
            qb.accessibility(self.db.W, self.db.delta)
            self.batches[qs] = qb
        return self.batches[qs], [self.ids[q] for q in qs]

    def ranked(self, n, cuts, opts=None, mask=None):
        """the queries cut into the batches `cuts` (tuples of query indices), in that order -> (the finished table's
        records, the restatement's bytes, the launches booked to "group" per searched page)"""
        from priblast_amd import capi
        recs, group_launches = [], []
        with capi.GroupRank(self.ctx, self.ng, n) as gr:
            for qs in cuts:
                qb, ids = self.batch(qs)
                o = opts() if opts else capi.default_opts()
                pm = mask(qb) if mask else None
                if pm:
                    o.allowed_pairs = pm.h.value
                try:
                    with capi.GroupSet(self.ctx, qb, self.db, self.maps, self.ng) as gs:
                        for p in range(self.db.npages):
                            before = self.ctx.stage_ms("group")[1]
                            gs.merge(p, o)
                            group_launches.append(self.ctx.stage_ms("group")[1] - before)
                        before = self.ctx.stage_ms("group")[1]
                        gr.add_groupset(gs, ids)
                        assert self.ctx.stage_ms("group")[1] == before  # (the merge books nothing to the group table's stage)
                        recs.append(grouprank_ref.with_ids(gs.finish(0), ids))
                finally:
                    if pm:
                        pm.close()
            return gr.finish(), grouprank_ref.rank_bytes(recs, n), group_launches

    def close(self):
        for qb in self.batches.values():
            qb.close()
        self.db.close()


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    c = Case(ctx, os.path.join(golden_dir, "mixdb"), seqs, 4)
    assert c.db.npages == 3 and any(c.maps[p][-1] == c.maps[p + 1][0] for p in range(2))  # a group spans two pages
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("grouprank_edge")
    refdump.unpack_case(GOLDEN, "edge", str(d))
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_q.fa"))
    c = Case(ctx, os.path.join(str(d), "edgedb"), seqs, 3)
    assert c.db.npages == 5
    yield c
    c.close()


def cuts_of(nq):
    """all queries in one batch; a batch per query; the same in reversed order"""
    whole, single = [tuple(range(nq))], [(q,) for q in range(nq)]
    return {"whole": whole, "single": single, "reversed": single[::-1]}


def check(case, n, **kw):
    got = {}
    for name, cuts in cuts_of(len(case.seqs)).items():
        recs, want, _ = case.ranked(n, cuts, **kw)
        assert recs.tobytes() == want, (n, name)
        got[name] = recs
    assert got["whole"].tobytes() == got["single"].tobytes() == got["reversed"].tobytes()
    return got["whole"]


@pytest.mark.parametrize("n", [1, 2, 64])
def test_mix_equals_the_restatement_however_the_queries_are_cut(mix, n):
    recs = check(mix, n)
    assert len(recs) > 3 and (recs["members"] > 1).any()
    assert np.bincount(recs["group"], minlength=mix.ng).max() <= n
    assert set(int(q) for q in recs["query"]) <= set(mix.ids)


def test_edge_equals_the_restatement_however_the_queries_are_cut(edge):
    recs = check(edge, 2)
    assert len(recs) > 0


def test_the_distinct_sites_and_the_chains(mix):
    from priblast_amd import capi
    plain = check(mix, 2)
    u = check(mix, 2, opts=lambda: capi.default_opts(distinct_sites=1))
    j = check(mix, 2, opts=lambda: capi.default_opts(chain_sites=1))
    assert len(u) == len(j) == len(plain)  # (a selection thins a pair's hits, never the pairs)
    # the distinct sites keep every pair's best hit: the same ranking, of fewer hits
    assert all(np.array_equal(u[k], plain[k]) for k in ("query", "group", "e_min", "rank")) and int(u["group_hits"].sum()) <= int(plain["group_hits"].sum())


def test_a_table_holds_one_selection(ctx, mix):
    from priblast_amd import capi
    qb, ids = mix.batch((0,))
    qb1, ids1 = mix.batch((1,))
    with capi.GroupRank(ctx, mix.ng, 2) as gr, capi.GroupRank(ctx, mix.ng, 2) as twin:
        for t in (gr, twin):
            with capi.GroupSet(ctx, qb, mix.db, mix.maps, mix.ng) as gs:
                for p in range(mix.db.npages):
                    gs.merge(p)
                t.add_groupset(gs, ids)
        for o in (capi.default_opts(distinct_sites=1), capi.default_opts(chain_sites=1)):
            with capi.GroupSet(ctx, qb1, mix.db, mix.maps, mix.ng) as gs:
                for p in range(mix.db.npages):
                    gs.merge(p, o)
                with pytest.raises(capi.PrbError, match="distinct_sites|chain_sites") as e:
                    gr.add_groupset(gs, ids1)
                assert "error -1:" in str(e.value)
        assert gr.counts() == twin.counts() and gr.counts()[2] > 0
        assert gr.finish().tobytes() == twin.finish().tobytes()


def test_under_a_pair_mask(ctx, mix):
    """every second target of the database allowed, for every query"""
    from priblast_amd import capi
    allowed = [(p, d) for p in range(mix.db.npages) for d in range(mix.db.page_info(p)[0])][::2]

    def mask(qb):
        pm = capi.PairMask(ctx, qb, mix.db)
        pm.allow(np.full(len(allowed), -1, np.int32), np.array([a[0] for a in allowed], np.int32), np.array([a[1] for a in allowed], np.int32))
        return pm

    masked = check(mix, 2, mask=mask)
    assert 0 < len(masked) and all((int(r["page"]), int(r["db_id"])) in allowed for r in masked)


def test_the_group_stage_launches_what_a_plain_group_run_launches(ctx, mix):
    """per searched page the "group" stage books what `-t -G` books for it: the merge into the ranking has a stage of
    its own"""
    from priblast_amd import capi
    cuts = cuts_of(len(mix.seqs))["whole"]
    _, _, with_rank = mix.ranked(2, cuts)
    qb, _ = mix.batch(cuts[0])
    plain = []
    with capi.GroupSet(ctx, qb, mix.db, mix.maps, mix.ng) as gs:
        for p in range(mix.db.npages):
            before = ctx.stage_ms("group")[1]
            gs.merge(p)
            plain.append(ctx.stage_ms("group")[1] - before)
        gs.finish(0)
    assert with_rank == plain and sum(plain) > 0
