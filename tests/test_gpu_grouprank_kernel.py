"""GPU tests of the group ranking table's kernels on hand-made records (prb_grouprank_*): through prb_groupset_add_pairs
and prb_grouprank_add_groupset on shape A of test_gpu_group_kernel.py - a 2-page database of 5 + 3 short targets - with 3
and with 130 queries, and through prb_grouprank_add_records.  The yardstick is tests/grouprank_ref.py's restatement, fed
with the exact records that prb_groupset_finish(gs, 0) returns; the table must match it byte for byte.  Nothing here
searches: the database and the batches only give the tables their shape."""
import itertools

import numpy as np
import pytest

import grouprank_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1

# groups of shape A: {t0, t5, t7} spans the pages, {t1, t2}, singletons t3, t4, t6
MAPS, NG = [[0, 1, 1, 2, 3], [0, 4, 0]], 5


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape(ctx, tmp_path_factory):
    """the database, and batches of 3, 2, 1 and 130 tiny queries"""
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    prefix = str(tmp_path_factory.mktemp("grouprank_db") / "gdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(8)], ["".join(rng.choice(list("ACGU"), 40)) for _ in range(8)], page_size=5)
    db = capi.Db(ctx, prefix)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == (5, 3)
    qbs = {nq: capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(nq)], db.repeat_flag) for nq in (3, 2, 1, 130)}
    yield db, qbs
    for qb in qbs.values():
        qb.close()
    db.close()


def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records with every other field filled in recognisably: from the row's
    place in the list, or from a fourth entry where the row has one"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for k, (q, d, e, *at) in enumerate(rows):
        i = at[0] if at else k
        out[k] = (q, d, 1 + (i + d) % 3, e, e - 1.5, 0.25 * i + d, e - 0.25 * i, (i, i + 1), (d + 2, d + 3))
    return out


def grecs(rows):
    """rows = [(identifier, group, e_min)] -> GROUP_DTYPE records as a caller's own fold would hand them in"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.GROUP_DTYPE)
    i = np.arange(len(rows))
    out["query"] = [r[0] for r in rows]
    out["group"] = [r[1] for r in rows]
    out["e_min"] = [r[2] for r in rows]
    out["db_id"] = out["group"] % 3
    out["hits"] = 1 + i % 3
    out["e_sum"] = out["e_min"] - 1.5
    out["e_acc"] = 0.25 * i
    out["e_hyb"] = out["e_min"] - 0.25 * i
    out["bp_first"] = np.stack([i, i + 1], 1)
    out["bp_last"] = np.stack([out["group"] + 2, out["group"] + 3], 1)
    out["members"] = 1 + i % 2
    out["group_hits"] = out["hits"] + out["members"]
    return out


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def groupset(ctx, db, qb, lists, skip_pages=()):
    """lists = {page: [(query, db_id, e_min)]} folded into a new group table; every page is merged (but skip_pages)"""
    from priblast_amd import capi
    gs = capi.GroupSet(ctx, qb, db, MAPS, NG)
    for p in range(db.npages):
        if p not in skip_pages:
            gs.add_pairs(p, pairs(lists.get(p, [])))
    return gs


def add(ctx, db, qb, gr, lists, ids):
    """a batch's lists through a group table into `gr`; -> the table's records under the identifiers, for the restatement:
    the group table is finished only after it was merged, which it must not notice"""
    with groupset(ctx, db, qb, lists) as gs:
        gr.add_groupset(gs, ids)
        return grouprank_ref.with_ids(gs.finish(0), ids)


def ranked(ctx, db, qbs, n, batches, order=None):
    """batches = [(lists, ids)] added in `order` -> (the finished table's bytes, the restatement's)"""
    from priblast_amd import capi
    with capi.GroupRank(ctx, NG, n) as gr:
        recs = [add(ctx, db, qbs[len(ids)], gr, lists, ids) for lists, ids in (batches if order is None else [batches[k] for k in order])]
        return gr.finish().tobytes(), grouprank_ref.rank_bytes(recs, n)


def test_one_record_and_more_slots_than_queries(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    got, want = ranked(ctx, db, qbs, 4, [({0: [(1, 3, -7.5)]}, [40, 41, 42])])
    assert got == want and len(got) == capi.GROUP_DTYPE.itemsize
    r = np.frombuffer(got, capi.GROUP_DTYPE)[0]
    assert (int(r["query"]), int(r["group"]), int(r["rank"]), float(r["e_min"]), int(r["members"])) == (41, 2, 0, -7.5, 1)
    # every query in every group, more slots than queries: everything is kept, ranked
    lists = {0: [(q, d, -5.0 - ((q + 2 * d) % 3)) for q in range(3) for d in range(5)], 1: [(q, d, -4.0 - (q + d) % 4) for q in range(3) for d in range(3)]}
    got, want = ranked(ctx, db, qbs, 7, [(lists, [9, 3, 6])])
    assert got == want and len(got) == 15 * capi.GROUP_DTYPE.itemsize


def test_the_best_of_three_candidates(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    got, want = ranked(ctx, db, qbs, 1, [({0: [(0, 0, -3.0), (1, 0, -9.0)], 1: [(2, 2, -4.0), (1, 0, -1.0)]}, [5, 6, 7])])
    assert got == want
    r = np.frombuffer(got, capi.GROUP_DTYPE)
    assert len(r) == 1 and (int(r[0]["query"]), int(r[0]["page"]), int(r[0]["members"])) == (6, 0, 2)


def test_an_empty_group_table_and_an_empty_table(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    got, want = ranked(ctx, db, qbs, 3, [({}, [0, 1, 2]), ({1: [(0, 1, -2.0)]}, [3, 4])])
    assert got == want and len(got) == capi.GROUP_DTYPE.itemsize
    with capi.GroupRank(ctx, NG, 3) as gr:
        assert len(gr.finish()) == 0
        assert len(gr.finish()) == 0  # (a second finish does nothing)
    with capi.GroupRank(ctx, NG, 3) as gr:
        gr.add_records(grecs([]))
        assert len(gr.finish()) == 0


def test_equal_energies_go_to_the_lower_identifier_whichever_batch_comes_first(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    batches = [({0: [(0, 1, -6.0), (1, 2, -6.0)], 1: [(1, 1, -6.0)]}, [7, 2]), ({0: [(0, 1, -6.0)], 1: [(0, 1, -6.0)]}, [4])]
    for n in (1, 2, 3):
        for order in ((0, 1), (1, 0)):
            got, want = ranked(ctx, db, qbs, n, batches, order)
            assert got == want, (n, order)
            r = np.frombuffer(got, capi.GROUP_DTYPE)
            assert [int(x["query"]) for x in r if x["group"] == 1] == [2, 4, 7][:n]


def test_the_two_zeros_tie_and_the_stored_bits_are_kept(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    batches = [({0: [(0, 0, 0.0), (1, 0, -0.0)]}, [8, 3]), ({0: [(0, 0, -0.0)]}, [5])]
    for order in ((0, 1), (1, 0)):
        got, want = ranked(ctx, db, qbs, 3, batches, order)
        assert got == want, order
        r = np.frombuffer(got, capi.GROUP_DTYPE)
        assert [(int(x["query"]), bool(np.signbit(x["e_min"]))) for x in r] == [(3, True), (5, True), (8, False)]


def wavefront_lists():
    """one add with 63, 64, 65 and 130 candidate queries in the groups 0 .. 3 (and 1 in group 4), energies with many ties"""
    rows = []
    for d, cnt in ((0, 63), (1, 64), (3, 65), (4, 130)):
        rows += [(q, d, -1.0 - ((q * 7 + d) % 13)) for q in range(cnt)]
    return {0: rows, 1: [(129, 1, -3.0)]}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_candidate_counts_at_the_wavefront_edge(ctx, shape, n):
    db, qbs = shape
    ids = [3 * q + 1 for q in range(130)][::-1]
    got, want = ranked(ctx, db, qbs, n, [(wavefront_lists(), ids)])
    assert got == want


def test_the_same_counts_through_add_records(ctx, shape):
    from priblast_amd import capi
    rows = [(2 * q, g, -1.0 - ((q * 5 + g) % 11)) for g, cnt in ((0, 63), (1, 64), (2, 65), (4, 130)) for q in range(cnt)]
    recs = grecs(rows)
    for n in (1, 64, 200):
        with capi.GroupRank(ctx, NG, n) as gr:
            gr.add_records(recs[::-1])
            assert gr.finish().tobytes() == grouprank_ref.rank_bytes([recs], n), n


@pytest.mark.parametrize("n", [1, 64, 1024])
def test_refill_of_full_lists(ctx, shape, n):
    """the lists are filled to the brim by the first add; the later ones displace the tail, the middle and the head, or
    nothing at all"""
    from priblast_amd import capi
    cnt = n + 70
    first = grecs([(q, g, -100.0 - 2.0 * ((q * 37) % cnt)) for g in (1, 3) for q in range(cnt)])
    kept_hi, kept_lo = -100.0 - 2.0 * 70, -100.0 - 2.0 * (cnt - 1)  # (the energies that the full list spans)
    middle = grecs([(5000 + q, 1, 0.5 * (kept_hi + kept_lo) - 2.0 * q - 1.0) for q in range(max(1, n // 3))])
    head = grecs([(7000 + q, g, -1e6 - q) for g in (1, 3) for q in range(3)])
    nothing = grecs([(9000 + q, 3, -1.0) for q in range(130)])
    ties = grecs([(9500 + q, 1, float(first["e_min"].min())) for q in range(2)])
    adds = [first, middle, head, nothing, ties]
    with capi.GroupRank(ctx, NG, n) as gr:
        for a in adds:
            gr.add_records(a)
        got = gr.finish()
    assert got.tobytes() == grouprank_ref.rank_bytes(adds, n)
    assert len(got) == 2 * n
    # (with one slot the head takes it; else some of the records that went into the middle are still there)
    assert n == 1 or set(int(x) for x in middle["query"]) & set(int(x) for x in got["query"])


def test_batch_invariance(ctx, shape):
    """the same records cut into one, two and five adds, in every order of the adds"""
    from priblast_amd import capi
    rng = np.random.default_rng(5)
    rows = [(q, g, float(rng.integers(-9, 0))) for q in range(40) for g in range(NG) if rng.random() < 0.6]
    recs = grecs(rows)
    for n in (1, 3, 64):
        want = grouprank_ref.rank_bytes([recs], n)
        for cuts in (1, 2, 5) if n == 3 else (1, 2):  # (120 orders of five adds: for one n)
            parts = [recs[recs["query"] % cuts == k] for k in range(cuts)]
            for order in itertools.permutations(range(cuts)):
                with capi.GroupRank(ctx, NG, n) as gr:
                    for k in order:
                        gr.add_records(parts[k])
                    assert gr.finish().tobytes() == want, (n, cuts, order)


def test_batch_invariance_through_group_tables(ctx, shape):
    """three queries as one batch, and as batches of two and one in both orders"""
    db, qbs = shape
    rows = {0: [(q, d, -2.0 - ((q + d) % 3)) for q in range(3) for d in (0, 1, 2, 4)], 1: [(q, d, -3.0 - ((2 * q + d) % 3)) for q in range(3) for d in range(3)]}
    # (a cut record keeps its place in the whole list: the same record in every cut)
    cut = lambda qs: {p: [(qs.index(q), d, e, i) for i, (q, d, e) in enumerate(r) if q in qs] for p, r in rows.items()}
    for n in (1, 2, 5):
        whole, want = ranked(ctx, db, qbs, n, [(rows, [10, 11, 12])])
        assert whole == want
        for order in ((0, 1), (1, 0)):
            got, want2 = ranked(ctx, db, qbs, n, [(cut([0, 2]), [10, 12]), (cut([1]), [11])], order)
            assert got == want2 == whole, (n, order)


def test_merge_invariance(ctx, shape):
    from priblast_amd import capi
    rng = np.random.default_rng(6)
    recs = grecs([(q, g, float(rng.integers(-9, 0))) for q in range(150) for g in range(NG) if rng.random() < 0.7])
    halves = [recs[recs["query"] % 2 == k] for k in (0, 1)]
    for n in (1, 5, 64, 1024):
        want = grouprank_ref.rank_bytes([recs], n)
        for a, b in ((0, 1), (1, 0)):
            with capi.GroupRank(ctx, NG, n) as dst, capi.GroupRank(ctx, NG, n) as src:
                dst.add_records(halves[a])
                src.add_records(halves[b])
                dst.absorb(src)
                assert dst.finish().tobytes() == want, (n, a)
                assert len(src.finish()) == 0
    # into an empty table, and an empty table into a full one
    with capi.GroupRank(ctx, NG, 5) as dst, capi.GroupRank(ctx, NG, 5) as src, capi.GroupRank(ctx, NG, 5) as none:
        src.add_records(recs)
        dst.absorb(src)
        dst.absorb(none)
        src.add_records(halves[0])  # (src is empty but valid: its identifiers are free again)
        assert dst.finish().tobytes() == grouprank_ref.rank_bytes([recs], 5)
        assert src.finish().tobytes() == grouprank_ref.rank_bytes([halves[0]], 5)


def test_refusals_leave_the_table_as_it_was(ctx, shape):
    from priblast_amd import capi
    db, qbs = shape
    base = grecs([(q, g, -1.0 - q - g) for q in (20, 21, 22) for g in range(NG)])
    lists = {0: [(0, 0, -50.0), (1, 3, -60.0)], 1: [(2, 1, -70.0)]}
    with capi.GroupRank(ctx, NG, 2) as twin:
        twin.add_records(base)
        want = twin.finish().tobytes()
    other = capi.Context(0)
    try:
        with capi.GroupRank(ctx, NG, 2) as gr:
            gr.add_records(base)

            def refused(code, match, call):
                with pytest.raises(capi.PrbError, match=match) as e:
                    call()
                assert code_of(e) == code, str(e.value)

            with groupset(ctx, db, qbs[3], lists, skip_pages=(1,)) as gs:  # one page still unmerged
                refused(STATE, "page 1 is not merged", lambda: gr.add_groupset(gs, [1, 2, 3]))
            with groupset(ctx, db, qbs[3], lists) as gs:
                refused(ARG, "given twice", lambda: gr.add_groupset(gs, [1, 2, 1]))
                refused(ARG, "already merged", lambda: gr.add_groupset(gs, [1, 21, 3]))
                refused(ARG, "below 0", lambda: gr.add_groupset(gs, [1, -2, 3]))
                with capi.GroupRank(other, NG, 2) as foreign:
                    refused(ARG, "another context", lambda: capi._check(capi.lib().prb_grouprank_add_groupset(
                        other.h, foreign.h, gs.h, np.array([1, 2, 3], np.int32).ctypes.data)))
                refused(ARG, "another context", lambda: capi._check(capi.lib().prb_grouprank_add_groupset(
                    other.h, gr.h, gs.h, np.array([1, 2, 3], np.int32).ctypes.data)))
                gs.finish(0)
                refused(STATE, "finished", lambda: gr.add_groupset(gs, [1, 2, 3]))
            with capi.GroupSet(ctx, qbs[3], db, [[0, 1, 1, 2, 3], [0, 4, 5]], 6) as gs6:  # unequal group counts
                for p in range(2):
                    gs6.add_pairs(p, pairs(lists[p]))
                refused(ARG, "6 groups", lambda: gr.add_groupset(gs6, [1, 2, 3]))
            refused(ARG, "names group 5", lambda: gr.add_records(grecs([(1, 5, -1.0)])))
            refused(ARG, "below 0", lambda: gr.add_records(grecs([(1, 0, -1.0), (-1, 1, -1.0)])))
            refused(ARG, "given twice", lambda: gr.add_records(grecs([(1, 0, -1.0), (2, 1, -1.0), (1, 0, -3.0)])))
            refused(ARG, "already merged", lambda: gr.add_records(grecs([(1, 0, -1.0), (22, 1, -99.0)])))
            with capi.GroupRank(ctx, NG, 3) as n3, capi.GroupRank(ctx, NG + 1, 2) as g6, capi.GroupRank(ctx, NG, 2) as shared:
                shared.add_records(grecs([(21, 0, -500.0), (30, 0, -500.0)]))
                refused(ARG, "records per group", lambda: gr.absorb(n3))
                refused(ARG, "groups", lambda: gr.absorb(g6))
                refused(ARG, "into both", lambda: gr.absorb(shared))
                assert len(shared.finish()) == 2  # (the refused source is as it was, too)
            assert gr.finish().tobytes() == want
            refused(STATE, "finished", lambda: gr.add_records(grecs([(1, 0, -1.0)])))
            with groupset(ctx, db, qbs[3], lists) as gs:
                refused(STATE, "finished", lambda: gr.add_groupset(gs, [1, 2, 3]))
            assert gr.finish().tobytes() == want
    finally:
        other.close()
    for n, ng in ((0, NG), (1025, NG), (2, 0)):
        with pytest.raises(capi.PrbError) as e:
            capi.GroupRank(ctx, ng, n)
        assert code_of(e) == ARG


def test_the_launches_of_the_grouprank_stage(ctx, shape):
    """7 per group table with occupied slots, 2 for an empty one, 5 per list of records, 1 per merge - and none booked to
    "group" but the group table's own"""
    from priblast_amd import capi
    db, qbs = shape
    with groupset(ctx, db, qbs[3], {0: [(0, 0, -1.0)]}) as gs, groupset(ctx, db, qbs[2], {}) as empty:
        ctx.reset_timers()
        with capi.GroupRank(ctx, NG, 2) as gr, capi.GroupRank(ctx, NG, 2) as src:
            gr.add_groupset(gs, [0, 1, 2])
            assert ctx.stage_ms("grouprank")[1] == 7
            gr.add_groupset(empty, [3, 4])
            assert ctx.stage_ms("grouprank")[1] == 9
            src.add_records(grecs([(9, 0, -1.0)]))
            assert ctx.stage_ms("grouprank")[1] == 14
            gr.absorb(src)
            assert ctx.stage_ms("grouprank")[1] == 15
            gr.finish()
        assert ctx.stage_ms("group")[1] == 0
