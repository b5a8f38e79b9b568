"""GPU tests of the feature null table over the ranked cut (prb_fnullset_create_top) on hand-made lists, as
test_gpu_fnull_kernel.py makes them: a 2-page database of 5 + 3 targets of 40 nt, 3 queries, 3 decoys each.  The yardstick
is the plain prb_fnullset_create table of the same lists under featuretop_ref.select: a kept record's null counts are those
of the uncut table.  Records are compared as bytes."""
import numpy as np
import pytest

import featuretop_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1
ND = 3

# target 0 of page 0: features 0 and 1 overlap, 2 is nested in 1, 3 repeats 0; target 1 has none; a feature on page 1
ANNOT = [(0, 0, 0, 19), (0, 0, 15, 30), (0, 0, 18, 20), (0, 0, 0, 19), (0, 2, 10, 20), (1, 1, 5, 15), (0, 4, 0, 39)]
# the real batch, {page: [(query, db_id, lo, hi, e_tot)]}: query 0 has the features 0 and 3 at -10, 1 at -9, 4 at -8 and 5 at
# -7, query 1 nothing, query 2 the features 6 and 5
REAL = {0: [(0, 0, 2, 5, -10.0), (0, 0, 25, 28, -9.0), (0, 2, 12, 14, -8.0), (2, 4, 0, 5, -0.5)], 1: [(0, 1, 5, 6, -7.0), (2, 1, 10, 12, -6.0)]}
# the decoys, {(owner, decoy): {page: [(db_id, lo, hi, e_tot)]}}; every other (owner, decoy) has no hit
DECOYS = {
    (0, 0): {0: [(0, 16, 19, -9.5),     # meets the features 0, 3 and 1: with n = 2 it counts in the kept 0 and 3 only
                 (0, 0, 1, -10.0)]},
    (0, 1): {0: [(1, 0, 39, -60.0),     # a target without features
                 (2, 20, 25, -8.0),     # only feature 4, which n <= 3 cuts away
                 (4, 3, 4, -50.0)]},    # only feature 6, which is kept for query 2 and not for query 0
    (0, 2): {0: [(2, 5, 10, -7.5)], 1: [(1, 15, 20, -7.0)]},  # the features 4 and 5: cut away with n <= 3
    (2, 0): {0: [(4, 1, 1, -0.75)]},
    (2, 1): {0: [(0, 0, 5, -40.0)], 1: [(1, 14, 20, -40.0)]},  # features kept for query 0 only; feature 5, kept for query 2 too
    (1, 0): {0: [(0, 0, 39, -20.0)], 1: [(1, 0, 39, -21.0)]},  # query 1 has no record at all
}
ALL = [(q, d) for q in range(3) for d in range(ND)]


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape(ctx, tmp_path_factory):
    from priblast_amd import capi
    rng = np.random.default_rng(23)
    seqs = ["".join(rng.choice(list("ACGU"), 40)) for _ in range(8)]
    prefix = str(tmp_path_factory.mktemp("ftopnulldb") / "fdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(8)], seqs, page_size=5)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(3)], db.repeat_flag)
    seqs_of = [[(db.seq_lengths(p, i)[2], db.seq_lengths(p, i)[0]) for i in range(db.page_info(p)[0])] for p in range(db.npages)]
    assert db.npages == 2 and [len(s) for s in seqs_of] == [5, 3]
    yield db, qb, seqs_of
    qb.close()
    db.close()


def make_hits(rows, seqs_page):
    """rows = [(query, db_id, lo, hi, e_tot)], [lo, hi] the hit's span in forward coordinates -> (HIT_DTYPE records with two
    pairs each, the pairs)"""
    from priblast_amd import capi
    hits = np.zeros(len(rows), capi.HIT_DTYPE)
    bp = np.zeros((2 * len(rows), 2), np.int32)
    for i, (q, d, lo, hi, e) in enumerate(rows):
        start_pos, length = seqs_page[d]
        t_lo, t_hi = start_pos + length - 1 - hi, start_pos + length - 1 - lo
        first, last = (t_lo, t_hi) if i % 2 else (t_hi, t_lo)
        bp[2 * i], bp[2 * i + 1] = (3 + i % 7, first), (9 + i % 5, last)
        h = hits[i]
        h["query"], h["db_id"], h["e_tot"], h["e_acc"], h["e_hyb"] = q, d, e, 0.125 * i + 1.0, e - 0.125 * i - 1.0
        h["bp_count"], h["bp_offset"] = 2, 2 * i
        h["q_sp"], h["db_sp"], h["q_len"], h["db_len"] = 3, t_lo, 7, hi - lo + 1
    return hits, bp


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def batch_hits(batch, page, seqs):
    """the hits of the batch's decoys against the page, `query` = the decoy's place in the batch, a decoy's hits by target"""
    rows = [(k, d, lo, hi, e) for k, key in enumerate(batch) for d, lo, hi, e in sorted(DECOYS.get(key, {}).get(page, []), key=lambda r: r[0])]
    return make_hits(rows, seqs[page])


def run(ctx, shape, batches, top=None, pages=(0, 1)):
    """the real lists into a feature table, that into a feature null table - over each query's `top` best records, if given -,
    the decoy batches in the order given -> (the finished records, the feature table's records)"""
    from priblast_amd import capi
    db, qb, seqs = shape
    with capi.Annotation(ctx, db, ANNOT) as an, capi.FeatSet(ctx, qb, an) as fs:
        for p in pages:
            fs.add_hits(p, *make_hits(REAL.get(p, []), seqs[p]))
        with capi.FNullSet(ctx, fs, ND, top) as fn:
            kept = capi.feature_records(fs)
            for batch in batches:
                fn.begin([o for o, _ in batch], [d for _, d in batch])
                for p in pages:
                    fn.add_hits(p, *batch_hits(batch, p, seqs))
                fn.end()
            return fn.finish(), kept


@pytest.fixture(scope="module")
def plain(ctx, shape):
    got, _ = run(ctx, shape, [ALL])  # computed once, never changed
    assert [(int(r["query"]), int(r["feature"])) for r in got] == [(0, 0), (0, 3), (0, 1), (0, 4), (0, 5), (2, 6), (2, 5)]
    assert got["null_hits"].tolist() == [1, 1, 1, 2, 1, 1, 1]  # every record has a decoy: a cut one's must count nowhere
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 1024])
def test_the_cut_table_is_the_plain_table_under_select(ctx, shape, plain, n):
    """n = 2 cuts query 0 behind its tie and keeps all of query 2; n = 1 cuts inside the tie"""
    from priblast_amd import capi
    want = featuretop_ref.select(plain, n)
    for batches, pages in (([ALL], (0, 1)), ([[k] for k in reversed(ALL)], (1, 0))):
        got, kept = run(ctx, shape, batches, n, pages)
        assert got.tobytes() == want.tobytes(), (n, got, want)
        for f in capi.FEATURE_DTYPE.names:  # the order and the records of prb_featset_records: the ranked ones
            assert got[f].tobytes() == kept[f].tobytes(), f
    assert [int((want["query"] == q).sum()) for q in range(3)] == [min(n, 5), 0, min(n, 2)]
    if n == 2:
        assert [(int(r["query"]), int(r["feature"]), int(r["null_hits"]), int(r["null_le"])) for r in got] == \
            [(0, 0, 1, 1), (0, 3, 1, 1), (2, 5, 1, 1), (2, 6, 1, 1)]


def test_create_top_guards(ctx, shape, plain):
    from priblast_amd import capi
    db, qb, seqs = shape
    with capi.Annotation(ctx, db, ANNOT) as an, capi.FeatSet(ctx, qb, an) as fs:
        for p in (0, 1):
            fs.add_hits(p, *make_hits(REAL.get(p, []), seqs[p]))
        for n in (0, 1025):
            with pytest.raises(capi.PrbError) as e:
                capi.FNullSet(ctx, fs, ND, n)
            assert code_of(e) == ARG and "1 <= n <= 1024" in str(e.value)
        with pytest.raises(capi.PrbError) as e:
            capi.FNullSet(ctx, fs, 0, 2)
        assert code_of(e) == ARG
        with capi.FNullSet(ctx, fs, ND, 2):  # the refusals left the feature table whole
            kept = capi.feature_records(fs)
            want = featuretop_ref.select(plain, 2)
            assert len(kept) == 4 and all(kept[f].tobytes() == want[f].tobytes() for f in capi.FEATURE_DTYPE.names)
            with pytest.raises(capi.PrbError) as e:  # it is finished - with n = 2
                capi.FNullSet(ctx, fs, ND, 2)
            assert code_of(e) == STATE
            with pytest.raises(capi.PrbError) as e:
                fs.finish()
            assert code_of(e) == STATE
            assert fs.finish_top(2).tobytes() == kept.tobytes()
