"""GPU tests of the feature ranking table's kernels (prb_featrank_*) on hand-made records: through
prb_featrank_add_records under hand-made annotations of 2 to 5 features of the smallest golden database (quirk), and
through prb_featset_add_hits and prb_featrank_add_featset on a 2-page database of 5 + 3 short targets with batches of 3
and 2 queries.  The yardstick is tests/featrank_ref.py's fold, fed with the exact records that prb_featset_finish
returns; the table must match it byte for byte, all 88 bytes of every record.  Nothing here searches: the databases and
the batches only give the tables their shape."""
import os

import numpy as np
import pytest

import featrank_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def annots(ctx, golden_dir):
    """annotations of 2 .. 5 features of the quirk database: feature f lies on its f-th target, whatever its page"""
    from priblast_amd import capi
    db = capi.Db(ctx, os.path.join(golden_dir, "quirkdb"))
    targets = [(p, i) for p in range(db.npages) for i in range(db.page_info(p)[0])]
    assert len(targets) >= 5
    made = {nf: capi.Annotation(ctx, db, [(p, i, 0, min(4 + f, db.seq_lengths(p, i)[0] - 1)) for f, (p, i) in enumerate(targets[:nf])])
            for nf in (2, 3, 4, 5)}
    yield made
    for an in made.values():
        an.close()
    db.close()


def frecs(rows):
    """rows = [(identifier, feature, e_min)] -> FEATRANK_DTYPE records as a caller's own fold would hand them in, every
    other field filled in recognisably from the row's place; rank and reserved hold junk that the table must not keep"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.FEATRANK_DTYPE)
    i = np.arange(len(rows))
    out["query"] = [r[0] for r in rows]
    out["feature"] = [r[1] for r in rows]
    out["e_min"] = [r[2] for r in rows]
    out["db_id"] = out["feature"]
    out["hits"] = 1 + i % 3
    out["e_sum"] = out["e_min"] - 1.5
    out["e_acc"] = 0.25 * i
    out["e_hyb"] = out["e_min"] - 0.25 * i
    out["bp_first"] = np.stack([i, i + 1], 1)
    out["bp_last"] = np.stack([out["feature"] + 2, out["feature"] + 3], 1)
    out["inside"] = i % 2
    out["rank"], out["reserved"] = 99, 7
    return out


def table(ctx, an, n, adds):
    """the finished table of `adds` (lists of records) in that order"""
    from priblast_amd import capi
    with capi.FeatRank(ctx, an, n) as fr:
        for a in adds:
            fr.add_records(a)
        return fr.finish()


def check(ctx, an, n, adds):
    got = table(ctx, an, n, adds)
    assert got.tobytes() == featrank_ref.rank_bytes(adds, n), (n, got)
    return got


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


# ------------------------------------------------------------------------- add_records
def test_basic_lists(ctx, annots):
    """nfeat 3, n 2: feature 1 stays empty, feature 2 has fewer than n records, feature 0 has equal energies (the lower
    identifier first) - and the two zeros tie, the stored bits kept"""
    recs = frecs([(8, 0, -6.0), (2, 0, -6.0), (5, 0, -6.0), (4, 2, -1.0)])
    got = check(ctx, annots[3], 2, [recs])
    assert [(int(r["feature"]), int(r["query"]), int(r["rank"]), int(r["reserved"])) for r in got] == [(0, 2, 0, 0), (0, 5, 1, 0), (2, 4, 0, 0)]
    zeros = [frecs([(8, 0, 0.0), (3, 0, -0.0)]), frecs([(5, 0, -0.0)])]
    for adds in (zeros, zeros[::-1]):
        got = check(ctx, annots[3], 2, adds)
        assert [(int(r["query"]), bool(np.signbit(r["e_min"]))) for r in got] == [(3, True), (5, True)]
    assert len(table(ctx, annots[3], 2, [])) == 0 and len(table(ctx, annots[3], 2, [frecs([])])) == 0


@pytest.mark.parametrize("n", [1, 3, 64, 70])
def test_streaming_steps(ctx, annots, n):
    """63, 64, 65 and 130 candidates for one feature each in a single add: the 64-key steps of the merge"""
    rows = [(3 * q + 1, f, -1.0 - ((q * 7 + f) % 13)) for f, cnt in ((0, 63), (1, 64), (2, 65), (3, 130)) for q in range(cnt)]
    recs = frecs(rows)
    got = check(ctx, annots[4], n, [recs[::-1]])
    assert np.bincount(got["feature"], minlength=4).tolist() == [min(n, c) for c in (63, 64, 65, 130)]
    # ... and on top of lists that are part full already
    check(ctx, annots[4], n, [frecs([(1000 + q, f, -7.5) for f in range(4) for q in range(2)]), recs])


@pytest.mark.parametrize("n", [3, 64])
def test_full_lists(ctx, annots, n):
    """a full list and newcomers none of which beats its last key (the fast path: nothing changes), then one that does"""
    first = frecs([(q, f, -100.0 - q) for f in (0, 1) for q in range(n + 5)])
    worse = frecs([(500 + q, 0, -100.0 + q) for q in range(130)] + [(700, 1, -100.0 - 4.5)])
    base = check(ctx, annots[2], n, [first])
    same = check(ctx, annots[2], n, [first, worse])
    assert same.tobytes() == base.tobytes()
    one = frecs([(900 + q, 0, -1.0) for q in range(70)] + [(980, 0, -100.0 - 5.5)])
    got = check(ctx, annots[2], n, [first, worse, one])
    assert set(got["query"][got["feature"] == 0].tolist()) - set(base["query"].tolist()) == {980}
    assert got[got["feature"] == 1].tobytes() == base[base["feature"] == 1].tobytes()


def test_slot_reuse(ctx, annots):
    """n 2 and three adds, each of which pushes entries out: a newcomer takes the slot of an entry that left"""
    adds = [frecs([(q, f, -1.0 - q) for f in (0, 1) for q in range(3)]), frecs([(10 + q, f, -10.0 - q - f) for f in (0, 1) for q in range(2)]),
            frecs([(20, 0, -10.5), (21, 0, -50.0), (22, 1, -11.5)])]
    got = check(ctx, annots[2], 2, adds)
    assert [(int(r["feature"]), int(r["query"])) for r in got] == [(0, 21), (0, 11), (1, 11), (1, 22)]
    for k in (1, 2):
        check(ctx, annots[2], 2, adds[:k])


def test_largest_list(ctx, annots):
    """n 1024 - the largest LDS footprint - with 1,100 candidates for one of two features, then 200 more that displace"""
    rng = np.random.default_rng(3)
    first = frecs([(q, 1, float(rng.integers(-400, 0))) for q in range(1100)] + [(5, 0, -2.0)])
    more = frecs([(2000 + q, 1, -200.0 - q) for q in range(200)])
    got = check(ctx, annots[2], 1024, [first, more])
    assert np.bincount(got["feature"]).tolist() == [1, 1024]


def test_merge(ctx, annots):
    """per feature: the destination's list empty, the source's empty, both part full, and together over n"""
    from priblast_amd import capi
    n, an = 4, annots[4]
    dst_recs = frecs([(q, f, -2.0 - q - f) for f, cnt in ((1, 2), (2, 1), (3, 3)) for q in range(cnt)])
    src_recs = frecs([(100 + q, f, -2.5 - q) for f, cnt in ((0, 2), (2, 2), (3, 3)) for q in range(cnt)])
    want = featrank_ref.rank_bytes([dst_recs, src_recs], n)
    for a, b in ((dst_recs, src_recs), (src_recs, dst_recs)):
        with capi.FeatRank(ctx, an, n) as dst, capi.FeatRank(ctx, an, n) as src:
            dst.add_records(a)
            src.add_records(b)
            dst.merge(src)
            got = dst.finish()
            assert got.tobytes() == want
            assert len(src.finish()) == 0
    assert np.bincount(got["feature"]).tolist() == [2, 2, 3, 4]
    # n = 1024 through the join, into an empty table, and an empty table into a full one
    big = frecs([(q, f, -1.0 - (q * 11) % 97) for f in (0, 3) for q in range(700)])
    halves = [big[big["query"] % 2 == k] for k in (0, 1)]
    with capi.FeatRank(ctx, an, 1024) as dst, capi.FeatRank(ctx, an, 1024) as src, capi.FeatRank(ctx, an, 1024) as none:
        src.add_records(halves[0])
        dst.merge(src)
        dst.merge(none)
        src.add_records(halves[1])  # (src is empty but valid: its identifiers are free again)
        dst.merge(src)
        assert dst.finish().tobytes() == featrank_ref.rank_bytes([big], 1024)


def test_batching_invariance(ctx, annots):
    """the same 300 records in 1, 2 and 7 adds, in two orders of the adds"""
    rng = np.random.default_rng(5)
    rows = [(q, f, float(rng.integers(-9, 0))) for q in range(120) for f in range(5) if rng.random() < 0.6][:300]
    recs = frecs(rows)
    assert len(recs) == 300
    for n in (1, 3, 64):
        want = featrank_ref.rank_bytes([recs], n)
        for cuts in (1, 2, 7):
            parts = [recs[recs["query"] % cuts == k] for k in range(cuts)]
            for order in (parts, parts[::-1]):
                assert table(ctx, annots[5], n, order).tobytes() == want, (n, cuts)


def test_refusals_of_add_records_and_create(ctx, annots):
    from priblast_amd import capi
    base = frecs([(q, f, -1.0 - q - f) for q in (20, 21, 22) for f in range(3)])
    want = table(ctx, annots[3], 2, [base]).tobytes()

    def refused(code, match, call):
        with pytest.raises(capi.PrbError, match=match) as e:
            call()
        assert code_of(e) == code, str(e.value)

    with capi.FeatRank(ctx, annots[3], 2) as fr:
        fr.add_records(base)
        refused(ARG, "names feature 3", lambda: fr.add_records(frecs([(1, 3, -1.0)])))
        refused(ARG, "names feature -1", lambda: fr.add_records(frecs([(1, -1, -1.0)])))
        refused(ARG, "below 0", lambda: fr.add_records(frecs([(1, 0, -1.0), (-1, 1, -1.0)])))
        refused(ARG, "given twice", lambda: fr.add_records(frecs([(1, 0, -1.0), (2, 1, -1.0), (1, 0, -3.0)])))
        refused(ARG, "already merged", lambda: fr.add_records(frecs([(1, 0, -1.0), (22, 1, -99.0)])))
        with capi.FeatRank(ctx, annots[3], 3) as n3, capi.FeatRank(ctx, annots[4], 2) as f4, capi.FeatRank(ctx, annots[3], 2) as shared:
            shared.add_records(frecs([(21, 0, -500.0), (30, 0, -500.0)]))
            refused(ARG, "records per feature", lambda: fr.merge(n3))
            refused(ARG, "features", lambda: fr.merge(f4))
            refused(ARG, "into both", lambda: fr.merge(shared))
            assert len(shared.finish()) == 2  # (the refused source is as it was, too)
        assert fr.finish().tobytes() == want  # (and so is the table)
    for n in (0, 1025):
        with pytest.raises(capi.PrbError, match="1 <= n <= 1024") as e:
            capi.FeatRank(ctx, annots[3], n)
        assert code_of(e) == ARG
    with capi.Annotation(ctx, annots[3].db, []) as empty:
        with pytest.raises(capi.PrbError, match="no feature") as e:
            capi.FeatRank(ctx, empty, 2)
        assert code_of(e) == ARG


def test_finish(ctx, annots):
    from priblast_amd import capi
    recs = frecs([(1, 0, -2.0), (2, 1, -3.0)])
    with capi.FeatRank(ctx, annots[2], 2) as fr:
        fr.add_records(recs)
        first = fr.finish().tobytes()
        assert fr.finish().tobytes() == first == featrank_ref.rank_bytes([recs], 2)  # (a second finish is OK)
        with pytest.raises(capi.PrbError, match="finished") as e:
            fr.add_records(frecs([(5, 0, -1.0)]))
        assert code_of(e) == STATE
        assert fr.finish().tobytes() == first


# ------------------------------------------------------------------------- add_featset
@pytest.fixture(scope="module")
def shape(ctx, tmp_path_factory):
    """a 2-page database of 5 + 3 targets of 40 nt, batches of 3 and 2 tiny queries, and the sequences' (start_pos, length)"""
    from priblast_amd import capi
    rng = np.random.default_rng(23)
    prefix = str(tmp_path_factory.mktemp("featrank_db") / "fdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(8)], ["".join(rng.choice(list("ACGU"), 40)) for _ in range(8)], page_size=5)
    db = capi.Db(ctx, prefix)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == (5, 3)
    qbs = {nq: capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(nq)], db.repeat_flag) for nq in (3, 2)}
    seqs = [[(db.seq_lengths(p, i)[2], db.seq_lengths(p, i)[0]) for i in range(db.page_info(p)[0])] for p in range(db.npages)]
    yield db, qbs, seqs
    for qb in qbs.values():
        qb.close()
    db.close()


# features: target 1 of page 0 has a nested pair, target 3 one, target 2 of page 1 one; target 0 of page 1 has none
ANNOT = [(0, 1, 5, 25), (0, 3, 0, 39), (0, 1, 10, 15), (1, 2, 0, 10)]
LISTS3 = {0: [(0, 1, 11, 14, -5.0), (0, 1, 14, 22, -6.0), (0, 3, 2, 8, -4.0), (1, 1, 12, 13, -6.0), (1, 1, 30, 39, -3.0), (2, 3, 0, 39, -2.0)],
          1: [(0, 2, 8, 12, -1.0), (2, 0, 0, 5, -8.0), (2, 2, 3, 20, -9.0)]}
LISTS2 = {0: [(0, 1, 11, 12, -6.0), (1, 3, 5, 6, -4.5)], 1: [(1, 2, 0, 3, -9.0)]}


def make_hits(rows, seqs_page):
    """rows = [(query, db_id, lo, hi, e_tot)], [lo, hi] the hit's span in forward coordinates -> (HIT_DTYPE records with two
    pairs each, the pairs)"""
    from priblast_amd import capi
    hits = np.zeros(len(rows), capi.HIT_DTYPE)
    bp = np.zeros((2 * len(rows), 2), np.int32)
    for i, (q, d, lo, hi, e) in enumerate(rows):
        start_pos, length = seqs_page[d]
        t_lo, t_hi = start_pos + length - 1 - hi, start_pos + length - 1 - lo
        bp[2 * i], bp[2 * i + 1] = (3 + i % 7, t_hi), (9 + i % 5, t_lo)
        h = hits[i]
        h["query"], h["db_id"], h["e_tot"], h["e_acc"], h["e_hyb"] = q, d, e, 0.125 * i + 1.0, e - 0.125 * i - 1.0
        h["bp_count"], h["bp_offset"] = 2, 2 * i
        h["q_sp"], h["db_sp"], h["q_len"], h["db_len"] = 3, t_lo, 7, hi - lo + 1
    return hits, bp


def featset(ctx, shape, an, nq, lists, skip_pages=()):
    from priblast_amd import capi
    db, qbs, seqs = shape
    fs = capi.FeatSet(ctx, qbs[nq], an)
    for p in range(db.npages):
        if p not in skip_pages:
            fs.add_hits(p, *make_hits(lists.get(p, []), seqs[p]))
    return fs


def test_add_featset_against_the_fold_of_the_finished_records(ctx, shape):
    """two batches through their feature tables, in both orders: the ranking is the fold of what prb_featset_finish returns
    of each - finished only after it was merged, which it must not notice -, and the unassigned hits are summed"""
    from priblast_amd import capi
    batches = [(3, LISTS3, [9, 3, 6]), (2, LISTS2, [4, 7])]
    with capi.Annotation(ctx, shape[0], ANNOT) as an:
        for n in (1, 2, 5):
            for order in (batches, batches[::-1]):
                with capi.FeatRank(ctx, an, n) as fr:
                    recs, un = [], 0
                    for nq, lists, ids in order:
                        with featset(ctx, shape, an, nq, lists) as fs:
                            fr.add_featset(fs, ids)
                            recs.append(featrank_ref.with_ids(fs.finish(), ids))
                            un += fs.unassigned()
                    got = fr.finish()
                    assert got.tobytes() == featrank_ref.rank_bytes(recs, n), (n, got)
                    assert fr.unassigned() == un == 2 and fr.counts() == (0, 0, 0)
        assert sum(len(r) for r in recs) == 12 and len(got) == 12
        # feature 0: -6.0 of the identifiers 9, 3 and 4: by identifier
        assert [int(r["query"]) for r in got if r["feature"] == 0] == [3, 4, 9]


def test_add_featset_refusals_and_an_empty_table(ctx, shape):
    from priblast_amd import capi

    def refused(code, match, call):
        with pytest.raises(capi.PrbError, match=match) as e:
            call()
        assert code_of(e) == code, str(e.value)

    with capi.Annotation(ctx, shape[0], ANNOT) as an, capi.Annotation(ctx, shape[0], ANNOT[:3] + [(1, 2, 0, 11)]) as other, \
            capi.Annotation(ctx, shape[0], list(ANNOT)) as equal:
        with featset(ctx, shape, an, 3, LISTS3) as twin, capi.FeatRank(ctx, an, 2) as fr0:
            fr0.add_featset(twin, [1, 2, 3])
            want = fr0.finish().tobytes()
        with capi.FeatRank(ctx, an, 2) as fr:
            with featset(ctx, shape, an, 3, LISTS3, skip_pages=(1,)) as fs:  # one page still unmerged
                refused(STATE, "page 1 is not merged", lambda: fr.add_featset(fs, [1, 2, 3]))
            with featset(ctx, shape, other, 3, LISTS3) as fs:
                refused(ARG, "different annotations", lambda: fr.add_featset(fs, [1, 2, 3]))
            with featset(ctx, shape, an, 3, LISTS3) as fs:
                refused(ARG, "given twice", lambda: fr.add_featset(fs, [1, 2, 1]))
                refused(ARG, "below 0", lambda: fr.add_featset(fs, [1, -2, 3]))
                fs.finish()
                refused(STATE, "finished", lambda: fr.add_featset(fs, [1, 2, 3]))
            # an empty but complete table is accepted, marks its identifiers and launches nothing
            ctx.reset_timers()
            with featset(ctx, shape, an, 2, {}) as empty:
                fr.add_featset(empty, [7, 8])
                assert ctx.stage_ms("featrank")[1] == 0
                refused(ARG, "already merged", lambda: fr.add_featset(empty, [8, 9]))
            # (a table of an equal annotation under another handle goes in)
            with featset(ctx, shape, equal, 3, LISTS3) as fs:
                fr.add_featset(fs, [1, 2, 3])
            assert fr.finish().tobytes() == want
            with featset(ctx, shape, an, 2, LISTS2) as fs:
                refused(STATE, "finished", lambda: fr.add_featset(fs, [4, 5]))


def test_the_launches_of_the_featrank_stage(ctx, shape):
    """5 per feature table with records, none for one without, 5 per list of records, none for an empty list, 1 per merge -
    and none booked to "feature" but the feature table's own"""
    from priblast_amd import capi
    with capi.Annotation(ctx, shape[0], ANNOT) as an, featset(ctx, shape, an, 3, LISTS3) as fs, featset(ctx, shape, an, 2, {}) as empty:
        ctx.reset_timers()
        with capi.FeatRank(ctx, an, 2) as fr, capi.FeatRank(ctx, an, 2) as src:
            fr.add_featset(fs, [0, 1, 2])
            assert ctx.stage_ms("featrank")[1] == 5
            fr.add_featset(empty, [3, 4])
            assert ctx.stage_ms("featrank")[1] == 5
            src.add_records(frecs([(9, 0, -1.0)]))
            assert ctx.stage_ms("featrank")[1] == 10
            src.add_records(frecs([]))
            assert ctx.stage_ms("featrank")[1] == 10
            fr.merge(src)
            assert ctx.stage_ms("featrank")[1] == 11
            fr.finish()
            assert ctx.stage_ms("featrank")[1] == 11
        assert ctx.stage_ms("feature")[1] == 0 and ctx.stage_ms("grouprank")[1] == 0
