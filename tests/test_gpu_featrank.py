"""GPU tests of the feature ranking table on the search path, on the `mix` fixture (3 pages) with the golden annotation
plus the three thirds of every target (the annot3 of test_gpu_featuretop.py): search_featrank - every batch searched into
a feature table of its own, which is merged into the ranking on the device - against featrank_ref.rank over the plain
finishes (prb_featset_finish) of the same searches, byte for byte.  All variants of one n - the queries in one batch, one
query per batch, the batches in reverse order, a page order of their own, several sub-batches - give identical bytes."""
import os

import numpy as np
import pytest

import feature_ref
import featrank_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NS = (1, 2, 1000)


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    """the database, the queries as one batch and as a batch each, the annotation, and - computed once, never changed -
    the plain finish of the whole batch under the default options, with distinct_sites = 1 and with chain_sites = 1"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
    assert db.npages == 3

    def batch(ss):
        qb = capi.QBatch(ctx, ss, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        return qb

    whole, singles = batch(seqs), [batch([s]) for s in seqs]
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        named = feature_ref.golden_annotation(f.read().splitlines()[2:])
    where, thirds = {}, []
    for p in range(db.npages):
        for i in range(db.page_info(p)[0]):
            where.setdefault(db.seq_name(p, i), (p, i))
            length = db.seq_lengths(p, i)[0]
            thirds += [(p, i, k * length // 3, (k + 1) * length // 3 - 1) for k in range(3)]
    an = capi.Annotation(ctx, db, [where[t] + (s, e) for t, s, e, _ in named] + thirds)
    ids = [3 * q + 2 for q in range(len(seqs))]  # (identifiers that are not the places in the batch)
    c = dict(db=db, an=an, whole=whole, singles=singles, ids=ids, full={}, unassigned={}, counts={})
    for key, opts in (("plain", {}), ("distinct", dict(distinct_sites=1)), ("chain", dict(chain_sites=1))):
        recs, un, counts = capi.search_features(ctx, whole, db, an, opts=capi.default_opts(**opts), with_counts=True)
        c["full"][key], c["unassigned"][key], c["counts"][key] = featrank_ref.with_ids(recs, ids), un, counts
    per_feature = np.bincount(c["full"]["plain"]["feature"])
    assert per_feature.max() > 2 and len(c["full"]["plain"]) >= 5  # n = 1 and n = 2 cut something
    assert len(c["full"]["distinct"]) and len(c["full"]["chain"])
    yield c
    an.close()
    for qb in [whole] + singles:
        qb.close()
    db.close()


def ranked(ctx, c, n, batches, **kw):
    from priblast_amd import capi
    return capi.search_featrank(ctx, c["db"], c["an"], n, batches, with_counts=True, **kw)


@pytest.mark.parametrize("n", NS)
def test_the_ranking_equals_the_fold_of_the_plain_finish_however_the_queries_are_batched(ctx, mix, n):
    full = mix["full"]["plain"]
    want = featrank_ref.rank_bytes([full], n)
    got, un, counts = ranked(ctx, mix, n, [(mix["whole"], mix["ids"])])
    assert got.tobytes() == want, (got, full)
    assert un == mix["unassigned"]["plain"] and counts == mix["counts"]["plain"]
    per_feature = np.bincount(full["feature"])
    assert len(got) == int(np.minimum(per_feature, n).sum()) and (n < 1000) == (len(got) < len(full))
    assert [(int(r["feature"]), int(r["rank"])) for r in got] == sorted((int(r["feature"]), int(r["rank"])) for r in got)
    each = [(qb, [mix["ids"][q]]) for q, qb in enumerate(mix["singles"])]
    for batches in (each, each[::-1]):
        again, un1, counts1 = ranked(ctx, mix, n, batches)
        assert again.tobytes() == want
        assert un1 == un and counts1[2] == counts[2]  # (the final hits; the earlier stages' counts are not compared across batchings)
    assert ranked(ctx, mix, n, [(mix["whole"], mix["ids"])], pages=[2, 0, 1])[0].tobytes() == want


def test_a_page_subset_is_refused_and_leaves_the_ranking_as_it_was(ctx, mix):
    """every identifier is merged exactly once, so a batch that was searched against some of the pages only cannot be
    ranked: prb_featrank_add_featset refuses its feature table (PRB_ERR_STATE), and the ranking table is as before"""
    from priblast_amd import capi
    with capi.FeatRank(ctx, mix["an"], 2) as fr:
        with capi.FeatSet(ctx, mix["whole"], mix["an"]) as fs:
            for p in (2, 0):
                fs.merge(mix["db"], p)
            with pytest.raises(capi.PrbError, match="page 1 is not merged") as e:
                fr.add_featset(fs, mix["ids"])
            assert int(str(e.value).split("error ")[1].split(":")[0]) == -5
            fs.merge(mix["db"], 1)  # (the feature table is as it was, too: its last page goes in, and then the table)
            fr.add_featset(fs, mix["ids"])
        assert fr.finish().tobytes() == featrank_ref.rank_bytes([mix["full"]["plain"]], 2)
    with pytest.raises(capi.PrbError, match="is not merged"):
        ranked(ctx, mix, 2, [(mix["whole"], mix["ids"])], pages=[2, 0])


def test_the_ranking_does_not_depend_on_sub_batches(ctx, mix, monkeypatch):
    monkeypatch.setenv("PRB_SEARCH_PAIRS", "1")  # (a query to a sub-batch)
    for n in NS:
        assert ranked(ctx, mix, n, [(mix["whole"], mix["ids"])])[0].tobytes() == featrank_ref.rank_bytes([mix["full"]["plain"]], n)


@pytest.mark.parametrize("key", ["distinct", "chain"])
def test_the_ranking_of_the_distinct_sites_and_of_the_chains(ctx, mix, key):
    from priblast_amd import capi
    opts = capi.default_opts(**{key + "_sites": 1})
    for n in NS:
        got, un, _ = ranked(ctx, mix, n, [(mix["whole"], mix["ids"])], opts=opts)
        assert got.tobytes() == featrank_ref.rank_bytes([mix["full"][key]], n) and un == mix["unassigned"][key]
    each = [(qb, [mix["ids"][q]]) for q, qb in enumerate(mix["singles"])]
    assert ranked(ctx, mix, 2, each[::-1], opts=opts)[0].tobytes() == featrank_ref.rank_bytes([mix["full"][key]], 2)
