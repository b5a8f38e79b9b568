"""GPU tests of the feature table's kernels on hand-made lists (prb_featset_add_hits runs the fold of
prb_search_page_features on a caller's hits): shape A, a 2-page database of 5 + 3 targets of 40 nt and 3 queries, and shape
B, 200 targets of 20 nt in pages of 64 and 2 queries.  The yardstick is tests/feature_ref.py's fold of the same lists;
records are compared as bytes.  Nothing here searches: the database and the batch only give the table its shape."""
import numpy as np
import pytest

import feature_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def build(ctx, tmp, ntargets, length, page_size, nq):
    from priblast_amd import capi
    rng = np.random.default_rng(23)
    seqs = ["".join(rng.choice(list("ACGU"), length)) for _ in range(ntargets)]
    prefix = str(tmp / "fdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(ntargets)], seqs, page_size=page_size)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(nq)], db.repeat_flag)
    seqs_of = [[(db.seq_lengths(p, i)[2], db.seq_lengths(p, i)[0]) for i in range(db.page_info(p)[0])] for p in range(db.npages)]
    return db, qb, seqs_of


@pytest.fixture(scope="module")
def shape_a(ctx, tmp_path_factory):
    db, qb, seqs = build(ctx, tmp_path_factory.mktemp("featdb_a"), 8, 40, 5, 3)
    assert db.npages == 2 and [len(s) for s in seqs] == [5, 3] and all(l == 40 for pg in seqs for _, l in pg)
    yield db, qb, seqs
    qb.close()
    db.close()


@pytest.fixture(scope="module")
def shape_b(ctx, tmp_path_factory):
    db, qb, seqs = build(ctx, tmp_path_factory.mktemp("featdb_b"), 200, 20, 64, 2)
    assert [len(s) for s in seqs] == [64, 64, 64, 8]
    yield db, qb, seqs
    qb.close()
    db.close()


def make_hits(rows, seqs_page):
    """rows = [(query, db_id, lo, hi, e_tot)], [lo, hi] the hit's span in forward coordinates -> (HIT_DTYPE records with two
    pairs each, the pairs); every other hit has its first pair at the span's other end, the other fields are recognisable"""
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


def run(ctx, db, qb, seqs, annot, lists, order=None):
    """lists = {page: rows of make_hits}, added in `order` (ascending by default) -> (records, unassigned, reference records,
    reference unassigned)"""
    from priblast_amd import capi
    pages = {p: make_hits(rows, seqs[p]) for p, rows in lists.items()}
    with capi.Annotation(ctx, db, annot) as an:
        assert an.count() == len(annot)
        with capi.FeatSet(ctx, qb, an) as fs:
            for p in (order if order is not None else sorted(pages)):
                fs.add_hits(p, *pages[p])
            got, un = fs.finish(), fs.unassigned()
    want, want_un = feature_ref.fold(pages, annot, seqs)
    return got, un, want, want_un


def check(ctx, shape, annot, lists, order=None):
    db, qb, seqs = shape
    got, un, want, want_un = run(ctx, db, qb, seqs, annot, lists, order)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert un == want_un
    return got, un


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def test_single_position_features_and_touching_spans(ctx, shape_a):
    # target 0: a feature of one position at forward 0, target 4 (the page's last): one at length - 1; target 2: [10, 20]
    annot = [(0, 0, 0, 0), (0, 4, 39, 39), (0, 2, 10, 20)]
    rows = [(0, 0, 0, 0, -9.0), (0, 0, 0, 5, -8.0), (0, 0, 1, 6, -7.0),               # on, across, one behind position 0
            (0, 2, 3, 9, -6.0), (0, 2, 3, 10, -6.5), (0, 2, 20, 25, -5.0), (0, 2, 21, 26, -4.0),  # one before / touching, both sides
            (0, 2, 12, 18, -3.0), (0, 2, 5, 30, -2.0),                                 # inside, and containing
            (0, 4, 39, 39, -9.5), (0, 4, 30, 38, -1.0)]
    got, un = check(ctx, shape_a, annot, {0: rows})
    assert un == 4  # the hits one position off, and the one that ends at 38
    by_feature = {int(r["feature"]): r for r in got}
    assert (int(by_feature[0]["hits"]), int(by_feature[0]["inside"])) == (2, 1)
    assert (int(by_feature[2]["hits"]), int(by_feature[2]["inside"])) == (4, 1)
    assert (int(by_feature[1]["hits"]), int(by_feature[1]["inside"])) == (1, 1)


def test_duplicate_nested_overlapping_and_a_gap_between_targets(ctx, shape_a):
    # target 1: the same feature twice, a nested and an overlapping one; target 2: none; target 3: one
    annot = [(0, 1, 5, 25), (0, 3, 0, 39), (0, 1, 10, 15), (0, 1, 5, 25), (0, 1, 20, 35), (1, 2, 0, 10)]
    lists = {0: [(0, 1, 11, 14, -5.0), (0, 1, 14, 22, -6.0), (0, 2, 1, 9, -7.0), (0, 3, 2, 8, -4.0), (1, 1, 30, 39, -3.0), (2, 3, 0, 39, -2.0)],
             1: [(0, 2, 8, 12, -1.0), (2, 2, 11, 20, -9.0), (2, 0, 0, 5, -8.0)]}
    got, un = check(ctx, shape_a, annot, lists)
    assert un == 3  # target 2 of page 0 and target 0 of page 1 have no feature; (2, 2, 11, 20) misses [0, 10]
    assert [(int(r["query"]), int(r["page"]), int(r["db_id"]), int(r["feature"])) for r in got] == \
        [(0, 0, 1, 0), (0, 0, 1, 3), (0, 0, 1, 2), (0, 0, 1, 4), (0, 0, 3, 1), (0, 1, 2, 5), (1, 0, 1, 4), (2, 0, 3, 1)]
    for order in ((1, 0),):
        again, _ = check(ctx, shape_a, annot, lists, order)
        assert again.tobytes() == got.tobytes()


def test_more_features_than_a_wavefront_on_one_target(ctx, shape_a):
    annot = [(1, 1, k % 33, k % 33 + k // 33 * 3) for k in range(70)]
    rows = [(1, 0, 0, 39, -1.0), (1, 1, 3, 4, -5.0), (1, 1, 30, 39, -6.0), (1, 1, 0, 39, -4.0), (1, 2, 5, 6, -2.0)]
    got, un = check(ctx, shape_a, annot, {1: rows})
    assert un == 2 and len(got) == 70 and len(set(got["feature"].tolist())) == 70


@pytest.mark.parametrize("nhits", [1, 65, 300])
def test_run_lengths(ctx, shape_b, nhits):
    """one run of 1, of 65 and of 300 hits (more than kFeatLongRun: the wavefront per item), on the first and on the last
    sequence of a page, with energies of magnitudes from 1e-8 to 1e16, so that a reassociated sum would show"""
    rng = np.random.default_rng(nhits)
    annot = [(1, 0, 0, 9), (1, 0, 5, 19), (1, 63, 2, 2), (1, 63, 0, 19), (1, 5, 0, 19)]
    rows = []
    for d in (0, 63):
        for i in range(nhits):
            lo = int(rng.integers(0, 20))
            hi = int(rng.integers(lo, 20))
            rows.append((1, d, lo, hi, float(-(10.0 ** rng.integers(-8, 9)) * rng.random()) if i % 3 else -1e16 + i))
    rows.sort(key=lambda r: r[1])
    got, un = check(ctx, shape_b, annot, {1: rows})
    assert len(got) >= 2 and un == 0
    seq = 0.0
    for r in rows:
        if r[1] == 63:
            seq += r[4]
    whole = [r for r in got if int(r["feature"]) == 3][0]  # the feature that is the whole of the page's last sequence
    assert int(whole["hits"]) == nhits and float(whole["e_sum"]) == seq


def test_fold_rules_first_minimum_and_signed_zero(ctx, shape_a):
    annot = [(0, 0, 0, 39), (0, 1, 0, 39), (0, 2, 0, 39)]
    rows = [(0, 0, 1, 2, -5.0), (0, 0, 3, 4, -7.0), (0, 0, 5, 6, -7.0), (0, 0, 7, 8, -6.0),  # equal minima: the first wins
            (0, 1, 1, 2, 0.0), (0, 1, 3, 4, -0.0),                                            # +0.0 then -0.0: +0.0 stays
            (0, 2, 1, 2, -0.0), (0, 2, 3, 4, 0.0),                                            # -0.0 then +0.0: -0.0 stays
            (1, 0, 1, 2, 1e16), (1, 0, 1, 2, 1.0), (1, 0, 1, 2, -1e16), (1, 0, 1, 2, 1.0)]    # (1e16 + 1) - 1e16 + 1 = 1, not 2
    got, un = check(ctx, shape_a, annot, {0: rows})
    assert un == 0
    assert got[0]["bp_first"].tolist() == make_hits(rows, shape_a[2][0])[1][2].tolist()  # the hit at index 1
    assert np.signbit(got[1]["e_min"]) == False and np.signbit(got[2]["e_min"]) == True  # noqa: E712
    assert float(got[3]["e_sum"]) == 1.0 and float(got[3]["e_min"]) == -1e16


def test_degenerate_inputs(ctx, shape_a):
    db, qb, seqs = shape_a
    rows = [(0, 0, 1, 2, -5.0), (2, 4, 3, 4, -7.0)]
    # no hits; an empty annotation; hits that all miss their features
    got, un = check(ctx, shape_a, [(0, 0, 0, 39)], {0: [], 1: []})
    assert len(got) == 0 and un == 0
    got, un = check(ctx, shape_a, [], {0: rows})
    assert len(got) == 0 and un == 2
    got, un = check(ctx, shape_a, [(0, 0, 10, 39), (0, 4, 0, 2), (0, 3, 0, 39)], {0: rows})
    assert len(got) == 0 and un == 2


def test_a_span_outside_its_sequence_is_refused_and_leaves_the_table(ctx, shape_a):
    from priblast_amd import capi
    db, qb, seqs = shape_a
    annot = [(0, 0, 0, 39), (0, 1, 0, 39)]
    good = [(0, 0, 1, 2, -5.0), (1, 1, 3, 4, -7.0)]
    with capi.Annotation(ctx, db, annot) as an, capi.FeatSet(ctx, qb, an) as fs:
        hits, bp = make_hits(good, seqs[0])
        bad_bp = bp.copy()
        bad_bp[3, 1] = seqs[0][1][0] + 40  # the separator behind target 1
        with pytest.raises(capi.PrbError) as e:
            fs.add_hits(0, hits, bad_bp)
        assert code_of(e) == STATE and "leaves its sequence" in str(e.value)
        bad_bp[3, 1] = seqs[0][1][0] - 1   # in front of it
        with pytest.raises(capi.PrbError) as e:
            fs.add_hits(0, hits, bad_bp)
        assert code_of(e) == STATE
        unsorted = hits[::-1].copy()
        with pytest.raises(capi.PrbError) as e:
            fs.add_hits(0, unsorted, bp)
        assert code_of(e) == ARG
        fs.add_hits(0, hits, bp)  # the page is still free, and the table whole
        with pytest.raises(capi.PrbError) as e:
            fs.add_hits(0, hits, bp)
        assert code_of(e) == ARG and "already merged" in str(e.value)
        got = fs.finish()
        assert got.tobytes() == feature_ref.fold({0: (hits, bp)}, annot, seqs)[0].tobytes() and len(got) == 2
        with pytest.raises(capi.PrbError) as e:
            fs.add_hits(1, *make_hits([], seqs[1]))
        assert code_of(e) == STATE


def test_annotation_refusals_name_the_entry(ctx, shape_a):
    from priblast_amd import capi
    db, qb, seqs = shape_a
    ok = (0, 0, 0, 39)
    for bad, word in (((2, 0, 0, 1), "page"), ((-1, 0, 0, 1), "page"), ((0, 5, 0, 1), "db_id"), ((1, 3, 0, 1), "db_id"),
                      ((0, 0, 5, 4), "start"), ((0, 0, -1, 4), "start"), ((0, 0, 0, 40), "length")):
        with pytest.raises(capi.PrbError) as e:
            capi.Annotation(ctx, db, [ok, ok, bad, (9, 9, 9, 9)])
        assert code_of(e) == ARG and "feature 2:" in str(e.value) and word in str(e.value), (bad, str(e.value))
    with capi.Annotation(ctx, db, []) as an:
        assert an.count() == 0
