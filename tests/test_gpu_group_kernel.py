"""GPU tests of the group table's kernels on hand-made lists (prb_groupset_add_pairs runs the fold of
prb_search_page_groups on a caller's records): shape A, a 2-page database of 5 + 3 short targets and 3 queries, and shape
B, 200 targets in pages of 64 and 2 queries, for the wavefront edges.  The yardstick is tests/group_ref.py's fold of the
same lists.  Nothing here searches: the database and the batch only give the table its shape."""
import itertools

import numpy as np
import pytest

import group_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def build(ctx, tmp, name, ntargets, length, page_size, nq):
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGU"), length)) for _ in range(ntargets)]
    prefix = str(tmp / name)
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(ntargets)], seqs, page_size=page_size)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(nq)], db.repeat_flag)
    return db, qb


# groups of shape A: {t0, t5, t7} spans the pages, {t1, t2}, singletons t3, t4, t6
MAPS_A, NG_A = [[0, 1, 1, 2, 3], [0, 4, 0]], 5


@pytest.fixture(scope="module")
def shape_a(ctx, tmp_path_factory):
    db, qb = build(ctx, tmp_path_factory.mktemp("groupdb_a"), "gdb", 8, 40, 5, 3)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == (5, 3)
    yield db, qb
    qb.close()
    db.close()


@pytest.fixture(scope="module")
def shape_b(ctx, tmp_path_factory):
    db, qb = build(ctx, tmp_path_factory.mktemp("groupdb_b"), "gdb", 200, 20, 64, 2)
    assert tuple(db.page_info(p)[0] for p in range(db.npages)) == (64, 64, 64, 8)
    yield db, qb
    qb.close()
    db.close()


@pytest.fixture(scope="module")
def shape_b128(ctx, tmp_path_factory):
    """the targets of shape B in pages of 128: a page of 64 holds at most 64 records of one query, a wavefront's worth; for
    more records than lanes on one slot in one launch the page has to be larger"""
    db, qb = build(ctx, tmp_path_factory.mktemp("groupdb_b128"), "gdb", 200, 20, 128, 2)
    assert tuple(db.page_info(p)[0] for p in range(db.npages)) == (128, 72)
    yield db, qb
    qb.close()
    db.close()


def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records with every other field filled in recognisably"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + (i + d) % 3, e, e - 1.5, 0.25 * i + d, e - 0.25 * i, (i, i + 1), (d + 2, d + 3))
    return out


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def run(ctx, db, qb, maps, ng, lists, n=0, order=None):
    """lists = {page: [(query, db_id, e_min)]}, added in `order` (ascending by default) -> the finished records"""
    from priblast_amd import capi
    with capi.GroupSet(ctx, qb, db, maps, ng) as gs:
        for p in (order if order is not None else sorted(lists)):
            gs.add_pairs(p, pairs(lists[p]))
        return gs.finish(n)


def ref(maps, ng, lists, n=0):
    return group_ref.fold({p: pairs(rows) for p, rows in lists.items()}, maps, ng, n)


# query 1 has no record; query 2 has the last target of the last page
LISTS_A = {0: [(0, 0, -10.0), (0, 1, -7.0), (0, 2, -9.0), (0, 4, -3.0), (2, 3, -8.0), (2, 1, -2.5)],
           1: [(0, 0, -12.0), (0, 2, -11.0), (0, 1, -1.0), (2, 2, -6.0), (2, 0, -6.5)]}


def test_plain_fold_equals_the_reference(ctx, shape_a):
    db, qb = shape_a
    got, want = run(ctx, db, qb, MAPS_A, NG_A, LISTS_A), ref(MAPS_A, NG_A, LISTS_A)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert [(int(r["query"]), int(r["group"])) for r in got] == [(0, 0), (0, 1), (0, 3), (0, 4), (2, 0), (2, 1), (2, 2)]
    r = got[0]
    assert (int(r["page"]), int(r["db_id"]), int(r["members"]), float(r["e_min"])) == (1, 0, 3, -12.0)
    assert int(r["group_hits"]) == sum(int(x["hits"]) for p in (0, 1) for x in pairs(LISTS_A[p]) if x["query"] == 0 and MAPS_A[p][x["db_id"]] == 0)
    assert 1 not in got["query"] and not got["rank"].any()


def test_ties_go_to_the_lower_page_then_the_lower_db_id(ctx, shape_a):
    db, qb = shape_a
    across = {0: [(0, 0, -5.0)], 1: [(0, 0, -5.0), (0, 2, -5.0)]}
    within = {0: [(1, 2, -4.0), (1, 1, -4.0)], 1: [(1, 2, -7.0), (1, 0, -7.0)]}
    for lists, best in ((across, (0, 0)), (within, (1, 0))):
        for order in ((0, 1), (1, 0)):
            got = run(ctx, db, qb, MAPS_A, NG_A, lists, order=order)
            assert got.tobytes() == ref(MAPS_A, NG_A, lists).tobytes(), (lists, order)
            assert (int(got[0]["page"]), int(got[0]["db_id"])) == best
    got = run(ctx, db, qb, MAPS_A, NG_A, within)
    assert [(int(r["group"]), int(r["page"]), int(r["db_id"])) for r in got] == [(0, 1, 0), (1, 0, 1)]


def test_the_two_zeros_tie_and_the_stored_bits_are_kept(ctx, shape_a):
    db, qb = shape_a
    for lists, neg in (({0: [(0, 0, 0.0)], 1: [(0, 0, -0.0), (0, 2, -0.0)]}, False), ({0: [(0, 0, -0.0)], 1: [(0, 0, 0.0)]}, True),
                       ({0: [(0, 2, 0.0), (0, 1, -0.0)]}, True)):
        for order in itertools.permutations(sorted(lists)):
            got = run(ctx, db, qb, MAPS_A, NG_A, lists, order=order)
            assert got.tobytes() == ref(MAPS_A, NG_A, lists).tobytes(), (lists, order)
            assert bool(np.signbit(got[0]["e_min"])) == neg and int(got[0]["page"]) == 0


def test_a_better_member_in_a_later_call_forgets_the_older_tie_key(ctx, shape_a):
    """page 0 leaves a tie key lower than any of page 1: a later, better member must win against it - and, the other way
    round, a later, worse member with a lower tie key must lose"""
    db, qb = shape_a
    lists = {0: [(0, 0, -5.0)], 1: [(0, 0, -9.0), (0, 2, -9.0)]}
    for order in ((0, 1), (1, 0)):
        got = run(ctx, db, qb, MAPS_A, NG_A, lists, order=order)
        assert got.tobytes() == ref(MAPS_A, NG_A, lists).tobytes(), order
        assert (int(got[0]["page"]), int(got[0]["db_id"]), float(got[0]["e_min"]), int(got[0]["members"])) == (1, 0, -9.0, 3)


def test_every_order_of_the_pages_gives_the_same_bytes(ctx, shape_b):
    db, qb = shape_b
    rng = np.random.default_rng(5)
    maps = [list(rng.integers(0, 9, 64)) for _ in range(3)] + [list(rng.integers(0, 9, 8))]
    lists = {p: [(q, d, float(rng.integers(-6, 0))) for q in range(2) for d in range(len(maps[p])) if rng.random() < 0.7] for p in range(4)}
    want = ref(maps, 9, lists).tobytes()
    for order in itertools.permutations(range(4)):
        assert run(ctx, db, qb, maps, 9, lists, order=order).tobytes() == want, order


def test_the_selection_keeps_each_querys_best_groups(ctx, shape_a):
    db, qb = shape_a
    hit = {q: len({MAPS_A[p][d] for p in LISTS_A for qq, d, _ in LISTS_A[p] if qq == q}) for q in (0, 2)}
    assert hit == {0: 4, 2: 3}
    for n in (0, 1, 3, 4, 5, 1024):
        got, want = run(ctx, db, qb, MAPS_A, NG_A, LISTS_A, n), ref(MAPS_A, NG_A, LISTS_A, n)
        assert got.tobytes() == want.tobytes(), (n, got, want)
        if n:
            assert [int(r["rank"]) for r in got] == [k for q in (0, 2) for k in range(min(n, hit[q]))]


def test_two_tables_over_split_pages_merge_to_the_bytes_of_one(ctx, shape_a):
    from priblast_amd import capi
    db, qb = shape_a
    for n in (0, 2):
        for first in (0, 1):
            with capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as a, capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as b:
                a.add_pairs(first, pairs(LISTS_A[first]))
                b.add_pairs(1 - first, pairs(LISTS_A[1 - first]))
                a.absorb(b)
                assert len(b.finish(0)) == 0
                assert a.finish(n).tobytes() == ref(MAPS_A, NG_A, LISTS_A, n).tobytes(), (n, first)


def test_merge_is_refused_for_unequal_maps_or_a_shared_page(ctx, shape_a):
    from priblast_amd import capi
    db, qb = shape_a
    other = [[0, 1, 1, 2, 3], [0, 4, 4]]
    with capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as a, capi.GroupSet(ctx, qb, db, other, NG_A) as b, \
            capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as c:
        a.add_pairs(0, pairs(LISTS_A[0]))
        b.add_pairs(1, pairs(LISTS_A[1]))
        c.add_pairs(0, pairs(LISTS_A[0]))
        c.add_pairs(1, pairs(LISTS_A[1]))
        with pytest.raises(capi.PrbError, match="different group maps") as e:
            a.absorb(b)
        assert code_of(e) == ARG
        with pytest.raises(capi.PrbError, match="page 0 is merged into both") as e:
            a.absorb(c)
        assert code_of(e) == ARG
        a.add_pairs(1, pairs(LISTS_A[1]))  # both tables are as they were
        assert a.finish().tobytes() == c.finish().tobytes() == ref(MAPS_A, NG_A, LISTS_A).tobytes()


def test_every_refusal_of_add_pairs_leaves_the_table_as_it_was(ctx, shape_a):
    from priblast_amd import capi
    db, qb = shape_a
    bad_hits = pairs([(0, 1, -3.0)])
    bad_hits["hits"] = 0
    with capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as gs:
        gs.add_pairs(0, pairs(LISTS_A[0]))
        for page, recs, what in ((1, pairs([(3, 0, -1.0)]), "out of range"), (1, pairs([(-1, 0, -1.0)]), "out of range"),
                                 (1, pairs([(0, 3, -1.0)]), "out of range"), (1, pairs([(0, -1, -1.0)]), "out of range"),
                                 (1, bad_hits, "out of range"), (1, pairs([(0, 1, -1.0), (1, 1, -2.0), (0, 1, -3.0)]), "has two records"),
                                 (0, pairs(LISTS_A[1]), "already merged"), (2, pairs([]), "out of range"), (-1, pairs([]), "out of range")):
            with pytest.raises(capi.PrbError, match=what) as e:
                gs.add_pairs(page, recs)
            assert code_of(e) == ARG, what
        gs.add_pairs(1, pairs(LISTS_A[1]))
        assert gs.finish().tobytes() == ref(MAPS_A, NG_A, LISTS_A).tobytes()


def test_nothing_is_added_after_finish_and_a_second_finish_does_nothing(ctx, shape_a):
    from priblast_amd import capi
    db, qb = shape_a
    with capi.GroupSet(ctx, qb, db, MAPS_A, NG_A) as gs:
        gs.add_pairs(0, pairs(LISTS_A[0]))
        with pytest.raises(capi.PrbError, match="need 0 <= n <= 1024") as e:
            gs.finish(1025)
        assert code_of(e) == ARG
        first = gs.finish(2)
        with pytest.raises(capi.PrbError, match="is finished") as e:
            gs.add_pairs(1, pairs(LISTS_A[1]))
        assert code_of(e) == STATE
        assert gs.finish(0).tobytes() == first.tobytes() == ref(MAPS_A, NG_A, {0: LISTS_A[0]}, 2).tobytes()


def test_create_checks_the_map(ctx, shape_a):
    from priblast_amd import capi
    db, qb = shape_a
    for maps, ng in (([[0, 1, 1, 2, 5], [0, 4, 0]], 5), ([[0, 1, 1, 2, -1], [0, 4, 0]], 5), (MAPS_A, 0), (MAPS_A, 9)):
        with pytest.raises(capi.PrbError) as e:
            capi.GroupSet(ctx, qb, db, maps, ng)
        assert code_of(e) == ARG


# ------------------------------------------------------------------------- shape B: the wavefront edges
def test_seventy_members_in_one_page_with_three_way_ties(ctx, shape_b128):
    """70 records on one slot in one launch - more than a wavefront has lanes, in two wavefronts of the launch - the minimum
    held by three of them; the second page ties with it again"""
    db, qb = shape_b128
    maps = [[0] * 70 + list(range(1, 59)), [0] * 2 + list(range(59, 129))]
    e = [-3.0 - (d % 5) for d in range(70)]
    for d in (66, 17, 40):
        e[d] = -20.0
    lists = {0: [(1, d, e[d]) for d in reversed(range(70))] + [(0, 9, -1.0), (1, 100, -20.0)], 1: [(1, 0, -4.0), (1, 1, -20.0)]}
    for order in ((0, 1), (1, 0)):
        got = run(ctx, db, qb, maps, 129, lists, order=order)
        assert got.tobytes() == ref(maps, 129, lists).tobytes(), order
        r = got[1]
        assert (int(r["query"]), int(r["group"]), int(r["page"]), int(r["db_id"]), int(r["members"])) == (1, 0, 0, 17, 72)


def test_a_full_wavefront_and_a_second_page_on_one_slot(ctx, shape_b):
    """pages of 64: every lane of a wavefront on one slot, the minimum held by three of them; a second page adds six
    members and ties with it again"""
    db, qb = shape_b
    maps = [[0] * 64, [0] * 6 + list(range(1, 59)), list(range(59, 123)), list(range(123, 131))]
    e = [-3.0 - (d % 5) for d in range(64)]
    for d in (61, 17, 40):
        e[d] = -20.0
    lists = {0: [(1, d, e[d]) for d in reversed(range(64))] + [(0, 9, -1.0)], 1: [(1, d, -20.0 if d == 2 else -4.0) for d in range(6)]}
    for order in ((0, 1), (1, 0)):
        got = run(ctx, db, qb, maps, 131, lists, order=order)
        assert got.tobytes() == ref(maps, 131, lists).tobytes(), order
        r = got[1]
        assert (int(r["query"]), int(r["group"]), int(r["page"]), int(r["db_id"]), int(r["members"])) == (1, 0, 0, 17, 70)


@pytest.mark.parametrize("n", [63, 64, 65, 129, 130])
def test_the_selection_among_130_groups(ctx, shape_b, n):
    db, qb = shape_b
    maps = [[0] * 64, [0] * 6 + list(range(1, 59)), list(range(59, 123)), list(range(123, 131))]
    rng = np.random.default_rng(n)
    # every group but one is hit by query 0 (130 groups), with many equal energies; query 1 hits 3 groups
    lists = {p: [(0, d, float(rng.integers(-9, -1))) for d in range(len(maps[p])) if maps[p][d] != 77] for p in range(4)}
    lists[2] += [(1, 0, -2.0), (1, 1, -2.0), (1, 63, -5.0)]
    got, want = run(ctx, db, qb, maps, 131, lists, n), ref(maps, 131, lists, n)
    assert len(want) == min(n, 130) + 3
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------- shape C: more groups than the selection sorts at once
@pytest.fixture(scope="module")
def shape_c(ctx, tmp_path_factory):
    db, qb = build(ctx, tmp_path_factory.mktemp("groupdb_c"), "gdb", 4300, 20, 2200, 2)
    assert tuple(db.page_info(p)[0] for p in range(db.npages)) == (2200, 2100)
    yield db, qb
    qb.close()
    db.close()


@pytest.mark.parametrize("n", [1, 1000, 1024])
def test_the_selection_refills_its_buffer(ctx, shape_c, n):
    """4300 groups of one target each, all hit by query 0: the workgroup of the selection sorts 2048 entries at a time, so it
    keeps its n best and refills the rest of its buffer twice (n = 1024: three times); the best groups lie in the last
    refill, ties everywhere; query 1 hits exactly 2048 groups - one full buffer, no refill"""
    db, qb = shape_c
    maps = [list(range(2200)), list(range(2200, 4300))]
    rng = np.random.default_rng(n)
    lists = {0: [(0, d, float(rng.integers(-40, -1))) for d in range(2200)] + [(1, d, float(rng.integers(-40, -1))) for d in range(2048)],
             1: [(0, d, float(rng.integers(-40, -1)) - (30.0 if d >= 2000 else 0.0)) for d in range(2100)]}
    got, want = run(ctx, db, qb, maps, 4300, lists, n), ref(maps, 4300, lists, n)
    assert len(want) == 2 * n
    assert got.tobytes() == want.tobytes()
