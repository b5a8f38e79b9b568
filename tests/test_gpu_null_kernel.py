"""GPU tests of the null table's two kernels on hand-made lists (prb_nullset_observe / prb_nullset_add_pairs run the
kernels of prb_search_page_observed / _decoys on a caller's records): a 2-page database of 5 + 3 short targets, 3
queries.  The yardstick is tests/null_ref.py's fold of the same lists.  Nothing here searches: the database and the
batch only give the table its shape."""
import numpy as np
import pytest

import null_ref

pytestmark = pytest.mark.gpu
NQ, NSEQ = 3, (5, 3)
STATE, ARG = -5, -1


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape(ctx, tmp_path_factory):
    """the database (pages of 5 and 3 targets of 40 nt) and a batch of 3 queries"""
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGU"), 40)) for _ in range(sum(NSEQ))]
    prefix = str(tmp_path_factory.mktemp("nulldb") / "ndb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(seqs))], seqs, page_size=5)
    db = capi.Db(ctx, prefix)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == NSEQ
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(NQ)], db.repeat_flag)
    yield db, qb
    qb.close()
    db.close()


def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records with every other field filled in recognisably"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + i % 3, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def run(ctx, db, qb, ndecoys, real, decoys, order=None):
    """real = {page: [(query, db_id, e_min)]}; decoys = [(page, owner[], decoy[], [(index, db_id, e_min)])] -> records"""
    from priblast_amd import capi
    with capi.NullSet(ctx, qb, db, ndecoys) as ns:
        for p in (0, 1):
            ns.observe(p, pairs(real.get(p, [])))
        for k in (order if order is not None else range(len(decoys))):
            page, owner, decoy, rows = decoys[k]
            ns.add_pairs(page, owner, decoy, pairs(rows))
        return ns.finish()


def ref(ndecoys, real, decoys):
    lists = []
    for page, owner, decoy, rows in decoys:
        recs = pairs(rows)
        for k in range(len(owner)):
            lists.append((owner[k], decoy[k], page, recs[recs["query"] == k]))
    merged = {}
    for o, d, page, recs in lists:
        merged.setdefault((o, d), {})[page] = recs
    return null_ref.fold({p: pairs(r) for p, r in real.items()}, [(o, d, pg) for (o, d), pg in merged.items()], ndecoys)


def all_decoys(ndecoys, rows_of):
    """every (owner, decoy) of both pages as one call per page; rows_of(page, owner, decoy) = [(db_id, e_min)]"""
    out = []
    for page in (0, 1):
        owner = [q for q in range(NQ) for _ in range(ndecoys)]
        decoy = [d for _ in range(NQ) for d in range(ndecoys)]
        rows = [(k, db_id, e) for k in range(len(owner)) for db_id, e in rows_of(page, owner[k], decoy[k])]
        out.append((page, owner, decoy, rows))
    return out


REAL = {0: [(0, 0, -10.0), (0, 3, -0.0), (1, 4, -12.5), (2, 1, -9.0)], 1: [(0, 2, -11.0), (2, 2, -8.25), (1, 0, -20.0)]}


def rows_mixed(page, owner, decoy):
    """ties, both zeros, weaker and stronger decoys, unobserved targets, the last target of the last page for query nq - 1"""
    if page == 0:
        r = {0: [(0, -10.0), (3, 0.0), (1, -30.0)],  # equal to the observed e_min: counts; +0.0 against -0.0: counts; (0, 1) is unobserved
             1: [(0, -9.5), (3, 1.0)],              # weaker; above zero
             2: [(0, -10.5), (4, -40.0)]}[decoy]    # stronger; (0, 4) is unobserved
        return r if owner == 0 else [(4, -12.5 - decoy)] if owner == 1 else []
    if owner == 2:
        return [(2, [-8.0, -8.25, -0.0][decoy])]     # the last target of the last page, query nq - 1
    return [(2, -11.0)] if owner == 0 and decoy == 1 else []


def test_counts_ties_zeros_and_unobserved_slots(ctx, shape):
    db, qb = shape
    decoys = all_decoys(3, rows_mixed)
    got, want = run(ctx, db, qb, 3, REAL, decoys), ref(3, REAL, decoys)
    assert got.tobytes() == want.tobytes(), (got, want)
    by = {(int(r["query"]), int(r["page"]), int(r["db_id"])): r for r in got}
    assert [tuple(k) for k in by] == sorted(by)  # by query, then page, then db_id
    assert len(by) == 7
    r = by[(0, 0, 0)]
    assert (r["null_hits"], r["null_le"], r["null_min"]) == (3, 2, -10.5)  # -10 (equal) and -10.5 count, -9.5 does not
    r = by[(0, 0, 3)]
    assert (r["null_hits"], r["null_le"]) == (2, 1) and r["null_min"].tobytes() == np.float64(0.0).tobytes()
    r = by[(2, 1, 2)]
    assert (r["null_hits"], r["null_le"], r["null_min"]) == (3, 1, -8.25)
    r = by[(1, 1, 0)]
    assert (r["null_hits"], r["null_le"]) == (0, 0) and np.isposinf(r["null_min"])
    assert all(r["decoys"] == 3 for r in got)


def test_4096_records_onto_one_slot(ctx, shape):
    db, qb = shape
    n = 4096
    real = {0: [(1, 2, -10.0)]}
    owner, decoy = [1] * n, list(range(n))
    e = -8.0 - (np.arange(n) % 5)  # -8 .. -12: three in five are <= -10
    rest = [(q, d) for q in (0, 2) for d in range(n)]
    decoys = [(0, owner, decoy, [(k, 2, float(e[k])) for k in range(n)]),
              (0, [q for q, _ in rest], [d for _, d in rest], []),
              (1, [q for q in range(NQ) for _ in range(n)], [d for _ in range(NQ) for d in range(n)], [])]
    got = run(ctx, db, qb, n, real, decoys)
    assert len(got) == 1
    assert (got[0]["null_hits"], got[0]["null_le"], got[0]["null_min"], got[0]["decoys"]) == (n, int((e <= -10.0).sum()), -12.0, n)
    assert int((e <= -10.0).sum()) == 2457
    assert got.tobytes() == ref(n, real, decoys).tobytes()


def test_empty_lists(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    none = all_decoys(2, lambda page, owner, decoy: [])
    assert len(run(ctx, db, qb, 2, {}, none)) == 0                    # n = 0 everywhere: no pair is observed
    got = run(ctx, db, qb, 2, REAL, none)                              # observed pairs, decoys without a hit
    assert got.tobytes() == ref(2, REAL, none).tobytes() and len(got) == 7
    assert (got["null_hits"] == 0).all() and np.isposinf(got["null_min"]).all()
    assert [null_ref.p_value(r) for r in got] == [1.0 / 3.0] * 7
    given = np.concatenate([pairs(REAL[0]), pairs(REAL[1])])           # `s` is the record given, field for field
    order = np.lexsort((given["db_id"], np.r_[np.zeros(4, int), np.ones(3, int)], given["query"]))
    for f in capi.PAIR_DTYPE.names:
        assert got[f].tobytes() == given[order][f].tobytes(), f


def test_two_orders_give_the_same_bytes(ctx, shape):
    db, qb = shape
    decoys = []
    for page in (0, 1):  # one call per (page, decoy number)
        for d in range(3):
            owner = list(range(NQ))
            rows = [(k, db_id, e) for k in range(NQ) for db_id, e in rows_mixed(page, owner[k], d)]
            decoys.append((page, owner, [d] * NQ, rows))
    a = run(ctx, db, qb, 3, REAL, decoys)
    b = run(ctx, db, qb, 3, REAL, decoys, order=[5, 0, 3, 4, 1, 2])
    c = run(ctx, db, qb, 3, REAL, all_decoys(3, rows_mixed))
    assert a.tobytes() == b.tobytes() == c.tobytes() and len(a) == 7


def test_refusals_leave_the_table_untouched(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    decoys = all_decoys(2, lambda page, owner, decoy: rows_mixed(page, owner, decoy))
    want = ref(2, REAL, decoys)
    with capi.NullSet(ctx, qb, db, 2) as ns:
        with pytest.raises(capi.PrbError) as e:  # decoys before the page is observed
            ns.add_pairs(0, [0], [0], pairs([]))
        assert code_of(e) == STATE and "not observed" in str(e.value)
        ns.observe(0, pairs(REAL[0]))
        ns.observe(1, pairs(REAL[1]))
        with pytest.raises(capi.PrbError) as e:  # a page observed twice
            ns.observe(1, pairs(REAL[1]))
        assert code_of(e) == ARG
        for owner, decoy, what in (([NQ], [0], "owner"), ([-1], [0], "owner"), ([0], [2], "decoy"), ([0], [-1], "decoy")):
            with pytest.raises(capi.PrbError) as e:
                ns.add_pairs(0, owner, decoy, pairs([(0, 0, -50.0)]))
            assert code_of(e) == ARG and what in str(e.value)
        with pytest.raises(capi.PrbError) as e:  # an (owner, decoy) twice in one call
            ns.add_pairs(0, [1, 1], [0, 0], pairs([(0, 4, -50.0)]))
        assert code_of(e) == ARG and "twice" in str(e.value)
        for rows in ([(1, 0, -50.0)], [(0, 5, -50.0)], [(0, -1, -50.0)], [(0, 0, -50.0), (0, 0, -51.0)]):
            with pytest.raises(capi.PrbError) as e:  # a record's query or db_id out of range; a pair with two records
                ns.add_pairs(0, [0], [0], pairs(rows))
            assert code_of(e) == ARG
        with pytest.raises(capi.PrbError) as e:  # a page out of range
            ns.add_pairs(2, [0], [0], pairs([]))
        assert code_of(e) == ARG
        with pytest.raises(capi.PrbError) as e:  # nothing of the decoys is in yet
            ns.finish()
        assert code_of(e) == STATE
        page, owner, decoy, rows = decoys[0]
        ns.add_pairs(page, owner, decoy, pairs(rows))
        with pytest.raises(capi.PrbError) as e:  # a (owner, decoy, page) given twice
            ns.add_pairs(0, [2], [1], pairs([(0, 1, -50.0)]))
        assert code_of(e) == ARG and "already merged" in str(e.value)
        with pytest.raises(capi.PrbError) as e:  # page 1's decoys are still missing
            ns.finish()
        assert code_of(e) == STATE and "6 of 12" in str(e.value)
        page, owner, decoy, rows = decoys[1]
        ns.add_pairs(page, owner, decoy, pairs(rows))
        got = ns.finish()
        assert got.tobytes() == want.tobytes()  # none of the refused calls left a trace
        assert len(ns.finish()) == len(want)    # a second finish does nothing
        with pytest.raises(capi.PrbError) as e:
            ns.observe(0, pairs([]))
        assert code_of(e) == STATE


def test_create_refuses_bad_decoy_counts(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    for n in (0, -1, 100001):
        with pytest.raises(capi.PrbError) as e:
            capi.NullSet(ctx, qb, db, n)
        assert code_of(e) == ARG and "ndecoys" in str(e.value)
