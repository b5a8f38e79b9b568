"""GPU tests of the sequential null table through the C ABI (prb_search_page_observed, prb_search_page_decoys,
prb_nullset_retire, prb_pairmask_create_live - capi.search_seqnull drives them as `ris -t -z N -H H -D R` does): the golden
mix database and queries against tests/seqnull_ref.py, whose per-decoy summaries come from capi.search_page_summary."""
import os

import numpy as np
import pytest

import null_ref
import refdump
import seqnull_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N, H, R, SEED = 6, 1, 2, 1


@pytest.fixture(scope="module")
def case(golden_dir):
    """the context, the database, the batch and its sequences, and the summaries of the real batch and of every decoy"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(HERE, "golden", "mix_q.fa"))
    with capi.Context(0) as ctx:
        db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        real, decoys = seqnull_ref.summaries(ctx, qb, seqs, db, N, seed=SEED)
        yield ctx, db, qb, seqs, real, decoys
        qb.close()
        db.close()


def test_the_reference_shows_every_case(case):
    real, decoys = case[4:]
    assert seqnull_ref.shows_every_case(real, decoys, N, H, R) == {"first": True, "later": True, "never": True, "differs": True}


def test_records_equal_the_reference_masked_and_unmasked(case):
    from priblast_amd import capi
    ctx, db, qb, seqs, real, decoys = case
    want = seqnull_ref.fold(real, decoys, N, H, R)
    got, counts, dcounts, rounds = capi.search_seqnull(ctx, qb, seqs, db, N, H, R, seed=SEED, with_counts=True)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert len(got) > 10 and set(got["decoys"].tolist()) == {2, 4, 6}
    # the live pairs after each round: the pairs that fewer than H of the decoys so far have reached
    for b, left in rounds:
        at = null_ref.fold(real, [x for x in decoys if x[1] < b], b)
        assert left.tolist() == [int(((at["query"] == q) & (at["null_le"] < H)).sum()) for q in range(len(seqs))], b
    assert [b for b, _ in rounds] == seqnull_ref.boundaries(N, R)
    plain, _, ucounts, urounds = capi.search_seqnull(ctx, qb, seqs, db, N, H, R, seed=SEED, mask=False, with_counts=True)
    assert plain.tobytes() == got.tobytes()
    assert all((a[1] == b[1]).all() for a, b in zip(rounds, urounds))
    assert 0 < dcounts[0] < ucounts[0]  # the mask dropped seeds
    # pieces that cut through an owner's round, and through the owners
    assert capi.search_seqnull(ctx, qb, seqs, db, N, H, R, seed=SEED, decoy_batch=3).tobytes() == got.tobytes()


def test_without_retiring_it_is_the_plain_null_table(case):
    from priblast_amd import capi
    ctx, db, qb, seqs, real, decoys = case
    want = null_ref.fold(real, decoys, N)
    assert capi.search_seqnull(ctx, qb, seqs, db, N, N, N, seed=SEED).tobytes() == want.tobytes()
    assert capi.search_null(ctx, qb, seqs, db, N, seed=SEED).tobytes() == want.tobytes()
