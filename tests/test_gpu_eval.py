"""GPU tests of the evalset end to end through the C ABI (prb_search_page_scored / prb_search_page_null_hits /
prb_evalset_close / prb_evalset_score) on the `mix` golden case, built in two pages, M = 3 decoys per query.

The yardstick is tests/eval_ref.py fed with the energies of plain prb_search_page runs of the same real batch and of
the same decoy batch (capi.null_decoys: the shuffles of `-z`), both pages.  The tee'd top-N hit table must be byte for
byte the one that prb_search_page_tophits fills alone.

OPTS: the default thresholds.  By the plain searches' own output they leave the fixture its teeth (33 real and 103
decoy hits; of the 23 kept hits 22 have NullLE > 0, one has NullLE = 0 and 20 have QValue < 1 - with distinct_sites the
decoys lose two hits and the kept hits' figures stay), so nothing looser was chosen; test_the_fixture_has_teeth asserts it."""
import os

import numpy as np
import pytest

import eval_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
M, SEED, FILE_POS0, KEEP = 3, 7, 2, 5
OPTS = {}


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mix2(ctx, tmp_path_factory):
    """mix in two pages: the database, the real batch, the decoy batch with its owners and decoy numbers"""
    from priblast_amd import capi
    tnames, targets = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    prefix = str(tmp_path_factory.mktemp("evalmix") / "mix2")
    capi.db_build(ctx, prefix, tnames, targets, page_size=(len(targets) + 1) // 2)
    db = capi.Db(ctx, prefix)
    assert db.npages == 2
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    dseqs, owner, decoy = capi.null_decoys(seqs, M, SEED, FILE_POS0)
    dqb = capi.QBatch(ctx, dseqs, db.repeat_flag)
    dqb.accessibility(db.W, db.delta)
    yield dict(db=db, qb=qb, dqb=dqb, owner=owner, decoy=decoy, nq=len(seqs))
    dqb.close()
    qb.close()
    db.close()


def options(distinct):
    from priblast_amd import capi
    return capi.default_opts(distinct_sites=distinct, **OPTS)


@pytest.fixture(scope="module")
def plain(ctx, mix2):
    """per distinct_sites: the (query, e_tot) of the real batch's final hits and the (owner, e_tot) of the decoys', from
    plain prb_search_page runs over both pages - computed once, never changed"""
    from priblast_amd import capi
    out = {}
    for distinct in (0, 1):
        o = options(distinct)
        rq, re_, dq, de = [], [], [], []
        for p in range(2):
            h = capi.search_page(ctx, mix2["qb"], mix2["db"], p, o)[0]
            rq.append(h["query"].copy()), re_.append(h["e_tot"].copy())
            h = capi.search_page(ctx, mix2["dqb"], mix2["db"], p, o)[0]
            dq.append(mix2["owner"][h["query"]]), de.append(h["e_tot"].copy())
        out[distinct] = tuple(np.concatenate(x) for x in (rq, re_, dq, de))
    return out


def scored(ctx, mix2, distinct, pages=(0, 1), decoy_first_page=0):
    """-> (tee'd records, tee'd base pairs, the kept hits' scores, the lists' sizes, the three sets of stage counts)"""
    from priblast_amd import capi
    o = options(distinct)
    with capi.EvalSet(ctx, mix2["qb"], mix2["db"], M) as es, capi.TopHits(ctx, mix2["qb"], KEEP) as th:
        for p in pages:
            es.scored(p, o, tophits=th)
        for p in (decoy_first_page, 1 - decoy_first_page):
            es.null_hits(mix2["dqb"], p, mix2["owner"], mix2["decoy"], o)
        es.finish()
        recs, bp = th.finish()
        return recs, bp, es.score(recs["query"], recs["e_tot"]), es.sizes(), es.counts(), es.decoy_counts(), th.counts()


def same(got, want):
    for f in ("decoys", "null_le", "rank", "q_num", "q_den"):
        assert np.array_equal(got[f].astype(np.int64), want[f]), f


@pytest.mark.parametrize("distinct", [0, 1], ids=["all_sites", "distinct_sites"])
def test_scores_equal_the_reference_and_the_tee_is_the_tophits_table(ctx, mix2, plain, distinct):
    from priblast_amd import capi
    rq, re_, dq, de = plain[distinct]
    recs, bp, got, sizes, counts, dcounts, tcounts = scored(ctx, mix2, distinct)
    assert sizes == (len(rq), len(dq)) and tcounts == counts
    if not distinct:  # (the stage counts are taken before the selection)
        assert counts[2] == len(rq) and dcounts[2] == len(dq)
    same(got, eval_ref.score(mix2["nq"], rq, re_, dq, de, M, look_q=recs["query"], look_e=recs["e_tot"]))
    alone, alone_bp, alone_counts = capi.search_tophits(ctx, mix2["qb"], mix2["db"], KEEP, options(distinct), with_counts=True)
    assert len(recs) > 0 and recs.tobytes() == alone.tobytes() and bp.tobytes() == alone_bp.tobytes() and tcounts == alone_counts
    # ... whatever the order of the pages
    recs2, bp2, got2, *_ = scored(ctx, mix2, distinct, pages=(1, 0), decoy_first_page=1)
    assert recs2.tobytes() == recs.tobytes() and bp2.tobytes() == bp.tobytes() and got2.tobytes() == got.tobytes()


def test_every_real_hit_equals_the_reference_without_a_tee(ctx, mix2, plain):
    from priblast_amd import capi
    rq, re_, dq, de = plain[0]
    with capi.EvalSet(ctx, mix2["qb"], mix2["db"], M) as es:
        for p in (0, 1):
            es.scored(p, options(0))
            es.null_hits(mix2["dqb"], p, mix2["owner"], mix2["decoy"], options(0))
        es.finish()
        same(es.score(rq, re_), eval_ref.score(mix2["nq"], rq, re_, dq, de, M))


@pytest.mark.parametrize("distinct", [0, 1], ids=["all_sites", "distinct_sites"])
def test_the_fixture_has_teeth(ctx, mix2, plain, distinct):
    """among the kept hits: one with NullLE > 0, one with QValue < 1, one with NullLE = 0 - from the plain searches alone"""
    from priblast_amd import capi
    rq, re_, dq, de = plain[distinct]
    alone, _ = capi.search_tophits(ctx, mix2["qb"], mix2["db"], KEEP, options(distinct))
    want = eval_ref.score(mix2["nq"], rq, re_, dq, de, M, look_q=alone["query"], look_e=alone["e_tot"])
    print("kept", len(alone), "real", len(rq), "decoy", len(dq), "null_le", want["null_le"].tolist(), "q", eval_ref.qvalue(want).tolist())
    assert (want["null_le"] > 0).any()
    assert (eval_ref.qvalue(want) < 1).any() and (want["null_le"] == 0).any()
    if distinct:
        assert len(dq) < len(plain[0][2])  # (the selection dropped hits)


def test_refusals_leave_the_tables_untouched(ctx, mix2):
    from priblast_amd import capi
    n = len(mix2["owner"])
    with capi.EvalSet(ctx, mix2["qb"], mix2["db"], M) as es, capi.TopHits(ctx, mix2["qb"], KEEP) as th:
        es.scored(0, options(0), tophits=th)
        with pytest.raises(capi.PrbError, match="already merged"):
            es.scored(0, options(0), tophits=th)
        with pytest.raises(capi.PrbError, match="distinct_sites"):
            es.scored(1, options(1), tophits=th)
        with pytest.raises(capi.PrbError, match="decoy"):
            es.null_hits(mix2["dqb"], 0, mix2["owner"], np.full(n, M))
        with pytest.raises(capi.PrbError, match="twice"):
            es.null_hits(mix2["dqb"], 0, np.zeros(n, int), np.zeros(n, int), options(0))
        with pytest.raises(capi.PrbError, match="are merged"):
            es.finish()
        es.null_hits(mix2["dqb"], 0, mix2["owner"], mix2["decoy"], options(0))
        with pytest.raises(capi.PrbError, match="already merged"):
            es.null_hits(mix2["dqb"], 0, mix2["owner"], mix2["decoy"], options(0))
        es.scored(1, options(0), tophits=th)
        es.null_hits(mix2["dqb"], 1, mix2["owner"], mix2["decoy"], options(0))
        es.finish()
        es.finish()  # (a second close does nothing)
        with pytest.raises(capi.PrbError, match="closed"):
            es.scored(1, options(0))
        recs, _ = th.finish()
        assert len(recs) > 0
    ms, launches = ctx.stage_ms("eval")
    assert ms > 0 and launches > 0
