"""GPU tests of the group null table on the search path (prb_search_page_gnull) through the C ABI, on the `mix` fixture:
its database has 3 pages, so groups span pages.  The decoys are made with prb_shuffle_sequence; the yardstick is
tests/gnull_ref.py's fold of capi.search_page_summary's plain, unmasked records of the real batch and of the decoys.
The table must match it byte for byte - with and without the decoys' pair mask, whatever the batches, with -n, and with
distinct_sites."""
import os

import pytest

import gnull_ref
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


def group_maps(db, per_group):
    """consecutive targets of the whole database, `per_group` to a group (so groups span the pages' borders)"""
    maps, t = [], 0
    for p in range(db.npages):
        nseq = db.page_info(p)[0]
        maps.append([(t + i) // per_group for i in range(nseq)])
        t += nseq
    return maps, (t + per_group - 1) // per_group


def summaries(ctx, seqs, db, opts):
    """the plain per-pair records of the batch `seqs` -> {page: records}"""
    from priblast_amd import capi
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    try:
        qb.accessibility(db.W, db.delta)
        return {p: capi.search_page_summary(ctx, qb, db, p, opts) for p in range(db.npages)}
    finally:
        qb.close()


def reference_input(ctx, seqs, db, opts):
    """the reference's input under `opts`: the real batch's records, and per decoy (owner, number, its records)"""
    from priblast_amd import capi
    dseqs, owner, decoy = capi.null_decoys(seqs, ND, SEED)
    real, dec = summaries(ctx, seqs, db, opts), summaries(ctx, dseqs, db, opts)
    decoys = [(int(owner[k]), int(decoy[k]), {p: r[r["query"] == k] for p, r in dec.items()}) for k in range(len(dseqs))]
    return real, decoys


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    assert db.npages == 3
    maps, ng = group_maps(db, 4)
    real, decoys = reference_input(ctx, seqs, db, capi.default_opts())  # computed once, never changed
    assert sum(len(r) for r in real.values()) > 10 and sum(len(r) for _, _, pages in decoys for r in pages.values()) > 0
    yield db, qb, seqs, maps, ng, real, decoys
    qb.close()
    db.close()


def test_the_table_equals_the_reference_fold_of_the_summaries(ctx, mix):
    from priblast_amd import capi
    db, qb, seqs, maps, ng, real, decoys = mix
    for n in (0, 2):
        want = gnull_ref.fold(real, maps, ng, decoys, ND, n)
        for mask in (True, False):
            got = capi.search_gnull(ctx, qb, seqs, db, maps, ng, ND, n, seed=SEED, mask=mask)
            assert got.tobytes() == want.tobytes(), (n, mask, got, want)
        if n == 0:  # no comparison of empty tables
            assert len(want) > 3 and (want["null_hits"] > 0).any() and (want["members"] > 1).any()
            assert (want["null_le"] <= want["null_hits"]).all() and (want["null_hits"] <= ND).all()


def test_the_table_does_not_depend_on_batches_or_page_order(ctx, mix):
    from priblast_amd import capi
    db, qb, seqs, maps, ng, real, decoys = mix
    want = gnull_ref.fold(real, maps, ng, decoys, ND, 2)
    got = capi.search_gnull(ctx, qb, seqs, db, maps, ng, ND, 2, seed=SEED, decoy_batch=5, pages=[2, 0, 1])
    assert got.tobytes() == want.tobytes()


def test_the_best_member_alone_is_another_statistic(ctx, mix):
    """a group of one target each: the columns are the per-pair null table's"""
    from priblast_amd import capi
    db, qb, seqs, _, _, real, decoys = mix
    maps, ng = group_maps(db, 1)
    got = capi.search_gnull(ctx, qb, seqs, db, maps, ng, ND, seed=SEED)
    assert got.tobytes() == gnull_ref.fold(real, maps, ng, decoys, ND).tobytes()
    pair = capi.search_null(ctx, qb, seqs, db, ND, seed=SEED)
    assert len(pair) == len(got)
    for f in ("query", "page", "db_id", "decoys", "null_hits", "null_le", "null_min"):
        assert got[f].tobytes() == pair[f].tobytes(), f


def test_with_distinct_sites(ctx, mix):
    from priblast_amd import capi
    db, qb, seqs, maps, ng, _, _ = mix
    opts = capi.default_opts(distinct_sites=1)
    real, decoys = reference_input(ctx, seqs, db, opts)
    want = gnull_ref.fold(real, maps, ng, decoys, ND)
    got = capi.search_gnull(ctx, qb, seqs, db, maps, ng, ND, seed=SEED, opts=opts)
    assert got.tobytes() == want.tobytes() and len(want) > 3
    # one selection per table: the decoys go with the one the group table was searched with
    with capi.GroupSet(ctx, qb, db, maps, ng) as gs:
        for p in range(db.npages):
            gs.merge(p, opts)
        with capi.GNullSet(ctx, gs, 0, 1) as gn:
            dseqs = [capi.shuffle_sequence(s, SEED, q, 0) for q, s in enumerate(seqs)]
            dqb, one = capi.QBatch(ctx, dseqs, db.repeat_flag), capi.QBatch(ctx, dseqs[:1], db.repeat_flag)
            try:
                dqb.accessibility(db.W, db.delta)
                one.accessibility(db.W, db.delta)
                gn.begin(list(range(len(seqs))), [0] * len(seqs))
                with pytest.raises(capi.PrbError) as e:
                    gn.merge(dqb, 0, capi.default_opts())
                assert "distinct_sites" in str(e.value)
                with pytest.raises(capi.PrbError) as e:  # a batch of another size than the open one
                    gn.merge(one, 0, opts)
                assert "decoys" in str(e.value)
            finally:
                dqb.close()
                one.close()
