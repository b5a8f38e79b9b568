"""GPU tests of the feature null table's kernels on hand-made lists: prb_featset_add_hits gives the real batch's records,
prb_fnullset_add_hits runs the fold of prb_search_page_fnull on a caller's decoy hits.  Shape: a 2-page database of 5 + 3
targets of 40 nt, 3 queries, 3 decoys each.  The yardstick is tests/fnull_ref.py's fold of the same lists; records are
compared as bytes.  Nothing here searches: the database and the batch only give the tables their shape."""
import numpy as np
import pytest

import fnull_ref
from test_gpu_feature_kernel import build, code_of, make_hits

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1
ND = 3

# target 0 of page 0: features 0 and 1 overlap, 2 is nested in 1, 3 repeats 0; target 1 has none; a feature on page 1
ANNOT = [(0, 0, 0, 19), (0, 0, 15, 30), (0, 0, 18, 20), (0, 0, 0, 19), (0, 2, 10, 20), (1, 1, 5, 15), (0, 4, 0, 39)]
# the real batch, {page: [(query, db_id, lo, hi, e_tot)]}: query 0 keeps features 0, 3, 1, 4 and 5, query 1 nothing, query 2
# keeps feature 6 at +0.0 and feature 5
REAL = {0: [(0, 0, 2, 5, -10.0), (0, 0, 25, 28, -9.0), (0, 2, 12, 14, -8.0), (2, 4, 0, 5, 0.0)], 1: [(0, 1, 5, 6, -7.0), (2, 1, 10, 12, -6.0)]}
# the decoys, {(owner, decoy): {page: [(db_id, lo, hi, e_tot)]}}; every other (owner, decoy) has no hit
DECOYS = {
    (0, 0): {0: [(0, 16, 19, -9.5),     # meets the overlapping features 0 (and 3) and 1: counted in each; above -10, below -9
                 (0, 0, 1, -10.0)]},    # ... and the minimum over the run's hits is equal to e_obs of feature 0
    (0, 1): {0: [(1, 0, 39, -60.0),     # a target without features
                 (2, 20, 25, -8.0),     # touches feature 4 by exactly its last position; equal to e_obs
                 (4, 3, 4, -50.0)]},    # only feature 6, which is kept for query 2 and not for query 0
    (0, 2): {0: [(2, 21, 25, -30.0), (2, 5, 10, -7.5), (2, 0, 9, -31.0)],  # misses by one, touches the first position, misses by one
             1: [(1, 15, 20, -7.0)]},   # page 1: touches feature 5 at its last position
    (2, 0): {0: [(4, 1, 1, -0.0)]},     # -0.0 against the observed +0.0
    (2, 1): {0: [(0, 0, 5, -40.0)], 1: [(1, 16, 20, -40.0)]},  # features kept for query 0 only; feature 5 missed by one
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
    db, qb, seqs = build(ctx, tmp_path_factory.mktemp("fnulldb"), 8, 40, 5, 3)
    assert db.npages == 2 and [len(s) for s in seqs] == [5, 3] and all(l == 40 for pg in seqs for _, l in pg)
    yield db, qb, seqs
    qb.close()
    db.close()


def batch_hits(decoys, batch, page, seqs):
    """the hits of the batch's decoys against the page, `query` = the decoy's place in the batch, a decoy's hits by target"""
    rows = [(k, d, lo, hi, e) for k, key in enumerate(batch) for d, lo, hi, e in sorted(decoys.get(key, {}).get(page, []), key=lambda r: r[0])]
    return make_hits(rows, seqs[page])


def real_pages(real, seqs):
    return {p: make_hits(real.get(p, []), seqs[p]) for p in range(len(seqs))}


def add_batch(fn, decoys, batch, seqs, pages=(0, 1)):
    fn.begin([o for o, _ in batch], [d for _, d in batch])
    for p in pages:
        fn.add_hits(p, *batch_hits(decoys, batch, p, seqs))
    fn.end()


def run(ctx, shape, batches, decoys=DECOYS, ndecoys=ND, pages=(0, 1), real=REAL, annot=ANNOT):
    """the real lists into a feature table, that into a feature null table, the decoy batches in the order given, every
    batch's pages in the order `pages` -> the finished records"""
    from priblast_amd import capi
    db, qb, seqs = shape
    with capi.Annotation(ctx, db, annot) as an, capi.FeatSet(ctx, qb, an) as fs:
        for p in pages:
            fs.add_hits(p, *real_pages(real, seqs)[p])
        with capi.FNullSet(ctx, fs, ndecoys) as fn:
            kept = capi.feature_records(fs)
            for batch in batches:
                add_batch(fn, decoys, batch, seqs, pages)
            got = fn.finish()
    for f in capi.FEATURE_DTYPE.names:  # the order and the records of prb_featset_records
        assert got[f].tobytes() == kept[f].tobytes(), f
    return got


def ref(shape, decoys=DECOYS, ndecoys=ND, real=REAL, annot=ANNOT):
    seqs = shape[2]
    batches = [({p: batch_hits(decoys, [key], p, seqs) for p in range(len(seqs))}, np.array([key[0]], np.int32), np.array([key[1]], np.int32))
               for key in decoys]
    return fnull_ref.fold_hits(real_pages(real, seqs), batches, annot, seqs, ndecoys)


def columns(recs):
    return [(int(r["query"]), int(r["feature"]), int(r["null_hits"]), int(r["null_le"]), float(r["null_min"])) for r in recs]


def test_the_counters_equal_the_reference(ctx, shape):
    got, want = run(ctx, shape, [ALL]), ref(shape)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert columns(got) == [(0, 0, 1, 1, -10.0), (0, 3, 1, 1, -10.0),  # the minimum of two hits of one run, equal to e_obs; the repeated feature
                            (0, 1, 1, 1, -9.5),                         # the same hit counted in the overlapping feature
                            (0, 4, 2, 1, -8.0),                         # touching at either end counts, one position off does not
                            (0, 5, 1, 1, -7.0),                         # the feature on page 1
                            (2, 6, 1, 1, 0.0),                          # -0.0 <= +0.0, reported as +0.0
                            (2, 5, 0, 0, np.inf)]                       # missed by one; the hits on query 0's features count nowhere
    assert not np.signbit(got[5]["null_min"]) and (got["decoys"] == ND).all() and not got["pad"].any()


BATCHINGS = {
    "one_decoy_per_batch": [[k] for k in ALL],
    "owners_interleaved": [[(q, d) for d in range(ND) for q in range(3)][i:i + 4] for i in range(0, 9, 4)],
    "batches_reversed": [[k] for k in reversed(ALL)],
    "seven_then_two": [ALL[:7], ALL[7:]],
}


@pytest.mark.parametrize("name", list(BATCHINGS))
def test_the_table_does_not_depend_on_the_batches(ctx, shape, name):
    assert run(ctx, shape, BATCHINGS[name]).tobytes() == ref(shape).tobytes()


def test_the_table_does_not_depend_on_the_order_of_the_pages(ctx, shape):
    for batches in ([ALL], BATCHINGS["owners_interleaved"]):
        assert run(ctx, shape, batches, pages=(1, 0)).tobytes() == ref(shape).tobytes()


def test_a_smaller_batch_counts_nothing_of_the_batch_before(ctx, shape):
    """7 decoys, then 2 whose first one - the first cells of the scratch, where decoy (0, 0) of the first batch stood - has no hit"""
    decoys = {k: v for k, v in DECOYS.items() if k != (0, 2)}
    first = [(0, 0), (0, 1), (2, 0), (2, 1), (2, 2), (1, 0), (1, 1)]
    got = run(ctx, shape, [first, [(0, 2), (1, 2)]], decoys=decoys)
    assert got.tobytes() == ref(shape, decoys).tobytes() and columns(got)[3] == (0, 4, 1, 1, -8.0)


@pytest.mark.parametrize("nhits", [129, 130, 200])
def test_long_runs_take_the_wavefront_form(ctx, shape, nhits):
    """one decoy with a run of more than kFeatLongRun = 128 hits on target 0, the minimum at the list positions 0, 63, 64, 128
    and the last; every fifth hit is lower still and lies outside the run's kept features"""
    for pos in (0, 63, 64, 128, nhits - 1):
        rows = []
        for i in range(nhits):
            if i == pos:
                rows.append((0, 3, 4, -11.0))
            elif i % 5 == 2:
                rows.append((0, 35, 39, -100.0 - i))
            else:
                rows.append((0, 0, 12, -1.0 - 0.125 * (i % 7)))
        decoys = {(0, 1): {0: rows}, (0, 0): {0: [(0, 0, 3, -2.0)]}}
        got = run(ctx, shape, [ALL], decoys=decoys)
        assert got.tobytes() == ref(shape, decoys).tobytes(), pos
        assert columns(got)[:3] == [(0, 0, 2, 1, -11.0), (0, 3, 2, 1, -11.0), (0, 1, 0, 0, np.inf)], pos


def test_many_decoys_of_one_owner_on_one_feature(ctx, shape):
    """200 decoys of query 0 in one batch, all with a hit in feature 4: a scratch of 200 x 5 cells, more than one workgroup
    per launch, and the atomics of several wavefronts on one record"""
    n = 200
    decoys = {(0, d): {0: [(2, 10 + d % 11, 30, -7.0 - 0.01 * d)] + ([(2, 0, 10, -7.99 - 0.001 * d)] if d % 2 else [])} for d in range(n)}
    rest = [(q, d) for q in (1, 2) for d in range(n)]
    got = run(ctx, shape, [[(0, d) for d in range(n)], rest], decoys=decoys, ndecoys=n)
    assert got.tobytes() == ref(shape, decoys, ndecoys=n).tobytes()
    assert columns(got)[3][:2] == (0, 4) and int(got[3]["null_hits"]) == n and 4 < int(got[3]["null_le"]) < n
    assert float(got[3]["null_min"]) == -7.0 - 0.01 * 199


def test_a_query_without_a_record_and_a_table_without_records(ctx, shape):
    got = run(ctx, shape, [ALL], real={0: [(1, 1, 0, 5, -3.0)]})  # (target 1 has no feature)
    assert len(got) == 0
    got = run(ctx, shape, [ALL[:3], ALL[3:6], ALL[6:]])  # the batch of query 1's decoys has no cell
    assert got.tobytes() == ref(shape).tobytes()


def test_refused_calls_leave_the_table_as_it_was(ctx, shape):
    from priblast_amd import capi
    db, qb, seqs = shape
    with capi.Annotation(ctx, db, ANNOT) as an:
        # a feature table with a page unmerged is refused, and stays usable
        fs = capi.FeatSet(ctx, qb, an)
        fs.add_hits(0, *real_pages(REAL, seqs)[0])
        with pytest.raises(capi.PrbError) as e:
            capi.FNullSet(ctx, fs, ND)
        assert code_of(e) == STATE
        fs.add_hits(1, *real_pages(REAL, seqs)[1])
        for nd in (0, 100001, -1):
            with pytest.raises(capi.PrbError) as e:
                capi.FNullSet(ctx, fs, nd)
            assert code_of(e) == ARG
        with fs, capi.FNullSet(ctx, fs, ND) as fn:
            with pytest.raises(capi.PrbError) as e:  # a finished feature table
                capi.FNullSet(ctx, fs, ND)
            assert code_of(e) == STATE
            with pytest.raises(capi.PrbError) as e:  # no batch is open
                fn.add_hits(0, *batch_hits(DECOYS, ALL, 0, seqs))
            assert code_of(e) == STATE
            with pytest.raises(capi.PrbError) as e:
                fn.end()
            assert code_of(e) == STATE
            for owner, decoy in (([0, 3], [0, 0]), ([0, 0], [0, ND]), ([0, 1, 0], [1, 1, 1])):  # out of range, out of range, twice
                with pytest.raises(capi.PrbError) as e:
                    fn.begin(owner, decoy)
                assert code_of(e) == ARG
            first, second = ALL[:3], ALL[3:]
            fn.begin([o for o, _ in first], [d for _, d in first])
            with pytest.raises(capi.PrbError) as e:  # begin while open
                fn.begin([o for o, _ in second], [d for _, d in second])
            assert code_of(e) == STATE
            fn.add_hits(0, *batch_hits(DECOYS, first, 0, seqs))
            with pytest.raises(capi.PrbError) as e:  # the page twice
                fn.add_hits(0, *batch_hits(DECOYS, first, 0, seqs))
            assert code_of(e) == ARG
            with pytest.raises(capi.PrbError) as e:  # a page outside the database
                fn.add_hits(2, *batch_hits(DECOYS, first, 0, seqs))
            assert code_of(e) == ARG
            with pytest.raises(capi.PrbError) as e:  # end with a page missing
                fn.end()
            assert code_of(e) == STATE
            with pytest.raises(capi.PrbError) as e:  # finish while open
                fn.finish()
            assert code_of(e) == STATE
            hits, bp = batch_hits(DECOYS, first, 1, seqs)
            assert len(hits) == 1
            for field, value in (("db_id", 3), ("db_id", -1), ("query", len(first)), ("bp_count", 0)):
                bad = hits.copy()
                bad[0][field] = value
                with pytest.raises(capi.PrbError) as e:
                    fn.add_hits(1, bad, bp)
                assert code_of(e) == ARG, field
            for off in (40, -1):  # a span that leaves its sequence: onto the separator behind it, and in front of it
                bad_bp = bp.copy()
                bad_bp[1, 1] = seqs[1][1][0] + off
                with pytest.raises(capi.PrbError) as e:
                    fn.add_hits(1, hits, bad_bp)
                assert code_of(e) == STATE and "leaves its sequence" in str(e.value)
            fn.add_hits(1, hits, bp)
            fn.end()
            with pytest.raises(capi.PrbError) as e:  # an (owner, decoy) of a batch closed before
                fn.begin([first[0][0]], [first[0][1]])
            assert code_of(e) == ARG
            with pytest.raises(capi.PrbError) as e:  # finish with decoys missing
                fn.finish()
            assert code_of(e) == STATE
            add_batch(fn, DECOYS, second, seqs)
            got = fn.finish()
            assert got.tobytes() == ref(shape).tobytes()
            assert fn.finish().tobytes() == got.tobytes()  # (a second call does nothing)
            with pytest.raises(capi.PrbError) as e:
                fn.begin([0], [0])
            assert code_of(e) == STATE


def test_the_stage_timer_counts_its_launches(ctx, shape):
    seqs = shape[2]
    ctx.reset_timers()
    batches = (ALL[:5], ALL[5:])
    run(ctx, shape, batches)
    ms, launches = ctx.stage_ms("fnull")
    with_features = {(p, d) for p, d, _, _ in ANNOT}
    folds = 0
    for batch in batches:
        for p in (0, 1):
            hits, _ = batch_hits(DECOYS, batch, p, seqs)
            if len(hits):  # head flags and the runs' selection, the items per run and their scan; with an item, the two folds
                folds += 4 + (2 if any((p, int(d)) in with_features for d in hits["db_id"]) else 0)
    # the keep, the sort and the check of the order; the folds; a close per batch with a cell; the gather
    assert launches == 3 + folds + 2 + 1 and ms > 0
