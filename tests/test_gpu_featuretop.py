"""GPU tests of the ranked cut of the feature table on the search path, on the `mix` fixture (3 pages) with the golden
annotation of test_gpu_feature.py: prb_search_page_features into two tables, prb_featset_finish_top of one against
featuretop_ref.select over the plain finish of the other, byte for byte; and the feature null table over the cut
(prb_fnullset_create_top), whose decoys are searched against the kept records' targets only."""
import os

import numpy as np
import pytest

import feature_ref
import featuretop_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ND, SEED = 4, 7


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    """the database, the batch, the golden annotation as (page, db_id, start, end) - and with the three thirds of every target
    behind it, so that decoys meet features -, and the plain finish of both: computed once, never changed"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        named = feature_ref.golden_annotation(f.read().splitlines()[2:])
    where, thirds = {}, []
    for p in range(db.npages):
        for i in range(db.page_info(p)[0]):
            where.setdefault(db.seq_name(p, i), (p, i))
            length = db.seq_lengths(p, i)[0]
            thirds += [(p, i, k * length // 3, (k + 1) * length // 3 - 1) for k in range(3)]
    c = dict(db=db, qb=qb, seqs=seqs, annot=[where[t] + (s, e) for t, s, e, _ in named])
    c["annot3"] = c["annot"] + thirds
    assert db.npages == 3
    for key in ("annot", "annot3"):
        with capi.Annotation(ctx, db, c[key]) as an:
            c["full_" + key] = capi.search_features(ctx, qb, db, an)[0]
        assert not (c["full_" + key]["e_min"] == 0).any()
    yield c
    qb.close()
    db.close()


def top(ctx, c, n, key="annot", pages=None):
    from priblast_amd import capi
    with capi.Annotation(ctx, c["db"], c[key]) as an, capi.FeatSet(ctx, c["qb"], an) as fs:
        for p in range(c["db"].npages) if pages is None else pages:
            fs.merge(c["db"], p)
        return fs.finish_top(n)


@pytest.mark.parametrize("n", [1, 2, 1024])
@pytest.mark.parametrize("key", ["annot", "annot3"])
def test_the_cut_equals_select_over_the_plain_finish(ctx, mix, key, n):
    full = mix["full_" + key]
    want = featuretop_ref.select(full, n)
    got = top(ctx, mix, n, key)
    assert got.tobytes() == want.tobytes(), (got, want)
    per_query = np.bincount(full["query"])
    assert per_query.max() > 2 and len(full) >= 5  # n = 1 and n = 2 cut something
    assert len(got) == int(np.minimum(per_query, n).sum()) and (n < 1024) == (len(got) < len(full))
    assert top(ctx, mix, n, key, pages=[2, 0, 1]).tobytes() == want.tobytes()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3"])
def test_the_cut_does_not_depend_on_sub_batches_or_chunks(ctx, mix, knob, monkeypatch):
    monkeypatch.setenv(*knob.split("="))  # (a query to a sub-batch; three hits to a chunk of the gapped stage)
    for n in (1, 2):
        assert top(ctx, mix, n, "annot3").tobytes() == featuretop_ref.select(mix["full_annot3"], n).tobytes()


def fnull(ctx, c, **kw):
    from priblast_amd import capi
    with capi.Annotation(ctx, c["db"], c["annot3"]) as an:
        return capi.search_fnull(ctx, c["qb"], c["seqs"], c["db"], an, ND, seed=SEED, with_counts=True, **kw)


def test_the_null_table_over_the_cut(ctx, mix):
    """the cut table's records are the plain table's under select, and its decoys - searched under the mask of the kept
    records' targets - pass no more seeds, ungapped and final hits than the plain run's"""
    n = 1
    full = mix["full_annot3"]
    targets = lambda recs: {(int(r["page"]), int(r["db_id"])) for r in recs}
    assert len(targets(featuretop_ref.select(full, n))) < len(targets(full))  # (the cut narrows the decoys' search space)
    plain, plain_counts = fnull(ctx, mix)
    want = featuretop_ref.select(plain, n)
    assert (plain["null_hits"] > 0).any()  # no comparison of empty nulls
    for mask in (True, False):
        got, counts = fnull(ctx, mix, top=n, mask=mask)
        assert got.tobytes() == want.tobytes(), (mask, got, want)
        if mask:
            print(counts, plain_counts)
            assert all(a <= b for a, b in zip(counts, plain_counts)), (counts, plain_counts)
    got, _ = fnull(ctx, mix, top=2, decoy_batch=5, pages=[2, 0, 1])
    assert got.tobytes() == featuretop_ref.select(plain, 2).tobytes()
