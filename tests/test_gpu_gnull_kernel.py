"""GPU tests of the group null table's kernels on hand-made lists: prb_groupset_add_pairs gives the real batch's records,
prb_gnullset_add_pairs runs the fold of prb_search_page_gnull on a caller's decoy records.  Shape: a 2-page database of
5 + 3 short targets, 3 queries, four groups.  The yardstick is tests/gnull_ref.py's fold of the same lists, field for
field, energies as bit patterns.  Nothing here searches: the database and the batch only give the tables their shape."""
import numpy as np
import pytest

import gnull_ref

pytestmark = pytest.mark.gpu
STATE, ARG = -5, -1

# group 0 = {page 0: t0, t1; page 1: t0} spans the pages, group 1 = {page 0: t2, t3}, group 2 = {page 0: t4} is a singleton,
# group 3 = {page 1: t1, t2} is never observed
MAPS, NG = [[0, 0, 1, 1, 2], [0, 3, 3]], 4
ND = 3
# the real batch, {page: [(query, db_id, e_min)]}: query 0 has groups 0 (-10.0, from page 0), 1 and 2; query 1 nothing;
# query 2 has group 0 through page 1 only, and group 1 at +0.0
REAL = {0: [(0, 0, -10.0), (0, 2, -9.0), (0, 4, -3.0), (2, 3, 0.0)], 1: [(0, 0, -8.0), (2, 0, -6.0)]}
# the decoys, {(owner, decoy): {page: [(db_id, e_min)]}}; every other (owner, decoy) has no hit
DECOYS = {
    (0, 0): {0: [(0, -11.0), (1, -12.0)], 1: [(1, -50.0)]},  # below e_obs on two members of group 0: once; group 3: nowhere
    (0, 1): {0: [(1, -10.0), (2, -30.0)]},                   # only on a member query 0 did not hit, and equal to e_obs; group 1
    (0, 2): {0: [(0, -9.5)], 1: [(0, -10.5)]},               # the minimum over group 0 is taken across the pages
    (2, 0): {0: [(3, -0.0)]},                                # -0.0 against the observed +0.0
    (2, 1): {0: [(4, -4.0)]},                                # group 2 is not observed for query 2: nowhere
    (1, 0): {0: [(0, -20.0)], 1: [(0, -21.0)]},              # query 1 has no group at all: nowhere
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
    rng = np.random.default_rng(11)
    prefix = str(tmp_path_factory.mktemp("gnulldb") / "gdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(8)], ["".join(rng.choice(list("ACGU"), 40)) for _ in range(8)], page_size=5)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(3)], db.repeat_flag)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == (5, 3)
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


def batch_records(decoys, batch, page):
    """the records of the batch's decoys against the page, `query` = the decoy's place in the batch"""
    return pairs([(k, d, e) for k, key in enumerate(batch) for d, e in decoys.get(key, {}).get(page, [])])


def group_table(ctx, db, qb, real=REAL, order=(0, 1)):
    from priblast_amd import capi
    gs = capi.GroupSet(ctx, qb, db, MAPS, NG)
    for p in order:
        gs.add_pairs(p, pairs(real.get(p, [])))
    return gs


def add_batch(gn, decoys, batch, pages=(0, 1)):
    gn.begin([o for o, _ in batch], [d for _, d in batch])
    for p in pages:
        gn.add_pairs(p, batch_records(decoys, batch, p))
    gn.end()


def run(ctx, shape, batches, decoys=DECOYS, ndecoys=ND, n=0, pages=(0, 1), real=REAL):
    """the real lists into a group table, that into a group null table under n, the decoy batches in the order given, every
    batch's pages in the order `pages` -> the finished records"""
    from priblast_amd import capi
    db, qb = shape
    with group_table(ctx, db, qb, real, pages) as gs, capi.GNullSet(ctx, gs, n, ndecoys) as gn:
        kept = capi.group_records(gs)
        for batch in batches:
            add_batch(gn, decoys, batch, pages)
        got = gn.finish()
    for f in capi.GROUP_DTYPE.names:  # the order and the records of prb_groupset_pairs
        assert got[f].tobytes() == kept[f].tobytes(), f
    return got


def ref(decoys=DECOYS, ndecoys=ND, n=0, real=REAL):
    return gnull_ref.fold({p: pairs(rows) for p, rows in real.items()}, MAPS, NG,
                          [(o, d, {p: pairs([(0, t, e) for t, e in rows]) for p, rows in pages.items()}) for (o, d), pages in decoys.items()],
                          ndecoys, n)


def columns(recs):
    return [(int(r["query"]), int(r["group"]), int(r["null_hits"]), int(r["null_le"]), float(r["null_min"])) for r in recs]


def test_the_counters_equal_the_reference(ctx, shape):
    got, want = run(ctx, shape, [ALL]), ref()
    assert got.tobytes() == want.tobytes(), (got, want)
    assert columns(got) == [(0, 0, 3, 3, -12.0),    # two members below e_obs count once; a member not hit; equal to e_obs; across pages
                            (0, 1, 1, 1, -30.0), (0, 2, 0, 0, np.inf),
                            (2, 0, 0, 0, np.inf),   # decoy (2, 1)'s record of group 2 and decoy (1, 0)'s are counted nowhere
                            (2, 1, 1, 1, 0.0)]      # -0.0 <= +0.0, reported as +0.0
    assert not np.signbit(got[4]["null_min"]) and (got["decoys"] == ND).all() and not got["pad"].any()


def test_with_n_the_groups_that_are_not_kept_count_nowhere(ctx, shape):
    got, want = run(ctx, shape, [ALL], n=1), ref(n=1)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert columns(got) == [(0, 0, 3, 3, -12.0), (2, 0, 0, 0, np.inf)]  # (query 2: -6.0 beats +0.0)


BATCHINGS = {
    "one_decoy_per_batch": [[k] for k in ALL],
    "owners_interleaved": [[(q, d) for d in range(ND) for q in range(3)][i:i + 4] for i in range(0, 9, 4)],
    "batches_reversed": [[k] for k in reversed(ALL)],
    "seven_then_two": [ALL[:7], ALL[7:]],
}


@pytest.mark.parametrize("name", list(BATCHINGS))
def test_the_table_does_not_depend_on_the_batches(ctx, shape, name):
    assert run(ctx, shape, BATCHINGS[name]).tobytes() == ref().tobytes()


def test_the_table_does_not_depend_on_the_order_of_the_pages(ctx, shape):
    for batches in ([ALL], BATCHINGS["owners_interleaved"]):
        assert run(ctx, shape, batches, pages=(1, 0)).tobytes() == ref().tobytes()
    only_page_1_first = {k: v for k, v in DECOYS.items() if k == (0, 2)}
    a, b = run(ctx, shape, [ALL], decoys=only_page_1_first, pages=(1, 0)), run(ctx, shape, [ALL], decoys=only_page_1_first)
    assert a.tobytes() == b.tobytes() == ref(only_page_1_first).tobytes() and columns(a)[0] == (0, 0, 1, 1, -10.5)


def test_a_smaller_batch_counts_nothing_of_the_batch_before(ctx, shape):
    """7 decoys, then 2 whose first one - cell 0 of the scratch, where decoy (0, 0) of the first batch stood - has no record"""
    decoys = {k: v for k, v in DECOYS.items() if k != (0, 2)}
    first = [(0, 0), (0, 1), (2, 0), (2, 1), (2, 2), (1, 0), (1, 1)]
    got = run(ctx, shape, [first, [(0, 2), (1, 2)]], decoys=decoys)
    assert got.tobytes() == ref(decoys).tobytes() and columns(got)[0] == (0, 0, 2, 2, -12.0)


def test_many_decoys_of_one_owner_on_one_group(ctx, shape):
    """200 decoys of query 0 in one batch, all with a hit in group 0 - on one, two or three of its members: a scratch of
    200 x 4 cells, more than one workgroup per launch, and the atomics of several wavefronts on one record"""
    n = 200
    decoys = {(0, d): {0: [(0, -5.0 - 0.01 * d)] + ([(1, -9.99 - 0.001 * d)] if d % 2 else []), **({1: [(0, -10.0)]} if d % 50 == 0 else {})}
              for d in range(n)}
    rest = [(q, d) for q in (1, 2) for d in range(n)]
    got = run(ctx, shape, [[(0, d) for d in range(n)], rest], decoys=decoys, ndecoys=n)
    want = ref(decoys, ndecoys=n)
    assert got.tobytes() == want.tobytes()
    assert int(got[0]["null_hits"]) == n and 4 < int(got[0]["null_le"]) < n and float(got[0]["null_min"]) == -9.99 - 0.001 * 199


def test_refused_calls_leave_the_table_as_it_was(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    # a group table with a page unmerged is refused, and stays usable
    gs = capi.GroupSet(ctx, qb, db, MAPS, NG)
    gs.add_pairs(0, pairs(REAL[0]))
    with pytest.raises(capi.PrbError) as e:
        capi.GNullSet(ctx, gs, 0, ND)
    assert code_of(e) == STATE
    gs.add_pairs(1, pairs(REAL[1]))
    for n, nd in ((0, 0), (0, 100001), (-1, ND), (1025, ND)):
        with pytest.raises(capi.PrbError) as e:
            capi.GNullSet(ctx, gs, n, nd)
        assert code_of(e) == ARG
    with gs, capi.GNullSet(ctx, gs, 0, ND) as gn:
        with pytest.raises(capi.PrbError) as e:  # no batch is open
            gn.add_pairs(0, batch_records(DECOYS, ALL, 0))
        assert code_of(e) == STATE
        for owner, decoy in (([0, 3], [0, 0]), ([0, 0], [0, ND]), ([0, 1, 0], [1, 1, 1])):  # out of range, out of range, twice
            with pytest.raises(capi.PrbError) as e:
                gn.begin(owner, decoy)
            assert code_of(e) == ARG
        first, second = ALL[:4], ALL[4:]
        gn.begin([o for o, _ in first], [d for _, d in first])
        with pytest.raises(capi.PrbError) as e:  # begin while open
            gn.begin([o for o, _ in second], [d for _, d in second])
        assert code_of(e) == STATE
        gn.add_pairs(0, batch_records(DECOYS, first, 0))
        with pytest.raises(capi.PrbError) as e:  # the page twice
            gn.add_pairs(0, batch_records(DECOYS, first, 0))
        assert code_of(e) == ARG
        with pytest.raises(capi.PrbError) as e:  # end with a page missing
            gn.end()
        assert code_of(e) == STATE
        with pytest.raises(capi.PrbError) as e:  # finish while open
            gn.finish()
        assert code_of(e) == STATE
        good = batch_records(DECOYS, first, 1)
        for field, value in (("db_id", 3), ("db_id", -1), ("query", len(first)), ("hits", 0)):
            bad = good.copy()
            bad[0][field] = value
            with pytest.raises(capi.PrbError) as e:
                gn.add_pairs(1, bad)
            assert code_of(e) == ARG, field
        with pytest.raises(capi.PrbError) as e:  # a (query, db_id) twice
            gn.add_pairs(1, np.concatenate([good, good[:1]]))
        assert code_of(e) == ARG
        gn.add_pairs(1, good)
        gn.end()
        with pytest.raises(capi.PrbError) as e:  # an (owner, decoy) of a batch closed before
            gn.begin([first[0][0]], [first[0][1]])
        assert code_of(e) == ARG
        with pytest.raises(capi.PrbError) as e:  # finish with decoys missing
            gn.finish()
        assert code_of(e) == STATE
        add_batch(gn, DECOYS, second)
        got = gn.finish()
        assert got.tobytes() == ref().tobytes()
        assert gn.finish().tobytes() == got.tobytes()  # (a second call does nothing)
        with pytest.raises(capi.PrbError) as e:
            gn.begin([0], [0])
        assert code_of(e) == STATE


def test_the_stage_timer_counts_its_launches(ctx, shape):
    ctx.reset_timers()
    run(ctx, shape, [ALL[:5], ALL[5:]])
    ms, launches = ctx.stage_ms("gnull")
    # the keep, per batch the folds of the pages with records and the close, the gather
    folds = sum(1 for batch in (ALL[:5], ALL[5:]) for p in (0, 1) if len(batch_records(DECOYS, batch, p)))
    assert launches == 1 + folds + 2 + 1 and ms > 0
