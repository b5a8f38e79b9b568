"""GPU tests of the feature null table on the search path (prb_search_page_fnull) through the C ABI, on the `mix` fixture
(3 pages).  The decoys are made with prb_shuffle_sequence; the yardstick is prb_search_page_features - existing code - run
on the real batch and on the batch of all decoys, unmasked, folded by tests/fnull_ref.py.  The annotation is the golden one
of test_gpu_feature.py with the three consecutive thirds of every target behind it, so that decoys meet features.  The
table must match the fold byte for byte - with and without the decoys' pair mask, whatever the batches, sub-batches and
chunks, with distinct_sites and with chain_sites."""
import os

import numpy as np
import pytest

import fnull_ref
from test_gpu_feature import load

pytestmark = pytest.mark.gpu
ND, SEED = 4, 7


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def decoy_features(ctx, c, annot, opts):
    """the feature records of the batch of all decoys under `opts`, and its owner and decoy columns"""
    from priblast_amd import capi
    dseqs, owner, decoy = capi.null_decoys(c["seqs"], ND, SEED)
    dqb = capi.QBatch(ctx, dseqs, c["db"].repeat_flag)
    try:
        dqb.accessibility(c["db"].W, c["db"].delta)
        with capi.Annotation(ctx, c["db"], annot) as an:
            recs, _ = capi.search_features(ctx, dqb, c["db"], an, opts)
    finally:
        dqb.close()
    return recs, owner, decoy


def reference(ctx, c, annot, opts=None):
    from priblast_amd import capi
    with capi.Annotation(ctx, c["db"], annot) as an:
        kept, _ = capi.search_features(ctx, c["qb"], c["db"], an, opts)
    return fnull_ref.fold_records(kept, [decoy_features(ctx, c, annot, opts)], ND)


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    c = load(ctx, golden_dir, "mix")
    assert c["db"].npages == 3
    thirds = [(p, d, k * length // 3, (k + 1) * length // 3 - 1) for p, pg in enumerate(c["seq_of"]) for d, (_, length) in enumerate(pg)
              for k in range(3)]
    c["annot3"] = c["annot"] + thirds
    c["want"] = reference(ctx, c, c["annot3"])  # computed once, never changed
    yield c
    c["qb"].close()
    c["db"].close()


def table(ctx, c, **kw):
    from priblast_amd import capi
    with capi.Annotation(ctx, c["db"], c["annot3"]) as an:
        return capi.search_fnull(ctx, c["qb"], c["seqs"], c["db"], an, ND, seed=SEED, **kw)


def test_the_table_equals_the_reference_fold_of_the_feature_tables(ctx, mix):
    want = mix["want"]
    for mask in (True, False):
        got = table(ctx, mix, mask=mask)
        assert got.tobytes() == want.tobytes(), (mask, got, want)
    # no comparison of empty tables
    assert len(want) > 10 and (want["null_hits"] > 0).any() and (want["null_hits"] == 0).any()
    assert (want["null_le"] <= want["null_hits"]).all() and (want["null_hits"] <= ND).all() and (want["decoys"] == ND).all()
    assert np.isinf(want["null_min"][want["null_hits"] == 0]).all() and np.isfinite(want["null_min"][want["null_hits"] > 0]).all()


def test_the_table_does_not_depend_on_batches_or_page_order(ctx, mix):
    got = table(ctx, mix, decoy_batch=5, pages=[2, 0, 1])
    assert got.tobytes() == mix["want"].tobytes()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3"])
def test_the_table_does_not_depend_on_sub_batches_or_chunks(ctx, mix, knob, monkeypatch):
    monkeypatch.setenv(*knob.split("="))  # (a query to a sub-batch; three hits to a chunk of the gapped stage)
    assert table(ctx, mix).tobytes() == mix["want"].tobytes()


@pytest.mark.parametrize("selection", ["distinct_sites", "chain_sites"])
def test_with_a_selection(ctx, mix, selection):
    from priblast_amd import capi
    opts = capi.default_opts(**{selection: 1})
    want = reference(ctx, mix, mix["annot3"], opts)
    got = table(ctx, mix, opts=opts)
    assert got.tobytes() == want.tobytes() and len(want) > 3
    # one selection per table: the decoys go with the one the feature table was searched with
    c = mix
    with capi.Annotation(ctx, c["db"], c["annot3"]) as an, capi.FeatSet(ctx, c["qb"], an) as fs:
        for p in range(c["db"].npages):
            fs.merge(c["db"], p, opts)
        with capi.FNullSet(ctx, fs, 1) as fn:
            dseqs = [capi.shuffle_sequence(s, SEED, q, 0) for q, s in enumerate(c["seqs"])]
            dqb, one = capi.QBatch(ctx, dseqs, c["db"].repeat_flag), capi.QBatch(ctx, dseqs[:1], c["db"].repeat_flag)
            try:
                dqb.accessibility(c["db"].W, c["db"].delta)
                one.accessibility(c["db"].W, c["db"].delta)
                fn.begin(list(range(len(dseqs))), [0] * len(dseqs))
                with pytest.raises(capi.PrbError) as e:
                    fn.merge(dqb, 0, capi.default_opts())
                assert selection in str(e.value)
                with pytest.raises(capi.PrbError) as e:  # a batch of another size than the open one
                    fn.merge(one, 0, opts)
                assert "decoys" in str(e.value)
            finally:
                dqb.close()
                one.close()
