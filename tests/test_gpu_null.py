"""GPU tests of the null table (prb_nullset_*, `ris -t -z N`) through the C ABI.  The yardstick is tests/null_ref.py:
the definition of include/priblast_hip.h folded in Python over capi.search_page_summary - pinned to the hit path by
test_gpu_summary.py - of the real batch and of every decoy of tests/shuffle_ref.py, each searched alone and unmasked.
The table must match it byte for byte."""
import os

import numpy as np
import pytest

import null_ref
import refdump
from test_gpu_options import OPTION_SETS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

RANDOM_SEED, RANDOM_SHUFFLE_SEED, RANDOM_DECOYS = 5, 3, 5


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def open_batch(ctx, prefix, seqs, max_resident_pages=None):
    from priblast_amd import capi
    db = capi.Db(ctx, prefix, max_resident_pages)
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    return db, qb


def assert_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


def random_case():
    """60 targets of 300 nt (three pages of 20) and three queries of 300 - 600 nt, all uniformly random.  With this seed
    and five decoys (shuffle seed RANDOM_SHUFFLE_SEED) the table has pairs of every kind - test_random_case_has_teeth says
    which; the seed was chosen with the CPU oracle (tests/oraclelib.py) before any GPU run."""
    rng = np.random.default_rng(RANDOM_SEED)
    letters = np.array(list("ACGU"))
    targets = ["".join(rng.choice(letters, 300)) for _ in range(60)]
    queries = ["".join(rng.choice(letters, int(n))) for n in rng.integers(300, 601, 3)]
    return [f"r{i}" for i in range(60)], targets, queries


# ------------------------------------------------------------------------- 1. the golden database
@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, "mixdb"), seqs)
    yield db, qb, seqs
    qb.close()
    db.close()


@pytest.mark.parametrize("opts", [{}, OPTION_SETS[1]], ids=["defaults", "f2_g5"])
def test_mix_equals_the_reference(ctx, mix, opts):
    from priblast_amd import capi
    db, qb, seqs = mix
    o = capi.default_opts(**opts)
    want = null_ref.null_ref(ctx, qb, seqs, db, 3, seed=7, file_pos0=2, opts=o)
    for mask in (True, False):
        got, counts, dcounts = capi.search_null(ctx, qb, seqs, db, 3, seed=7, file_pos0=2, opts=o, mask=mask, with_counts=True)
        assert_bytes(got, want, ("mix", opts, mask))
    assert len(got) > 0 and (got["decoys"] == 3).all()
    # `s` is the summary record, field for field
    summ = {(int(r["query"]), p, int(r["db_id"])): r for p in range(db.npages) for r in capi.search_page_summary(ctx, qb, db, p, o)}
    assert len(summ) == len(got)
    for r in got:
        s = summ[(int(r["query"]), int(r["page"]), int(r["db_id"]))]
        assert all(r[f].tobytes() == s[f].tobytes() for f in capi.PAIR_DTYPE.names)
    assert counts[2] == sum(int(r["hits"]) for r in got)


# ------------------------------------------------------------------------- 2. a random database in three pages
@pytest.fixture(scope="module")
def rnd(ctx, tmp_path_factory):
    """the random case built, its batch, and its reference table - computed once, never changed"""
    from priblast_amd import capi
    names, targets, queries = random_case()
    prefix = str(tmp_path_factory.mktemp("rnd") / "rdb")
    capi.db_build(ctx, prefix, names, targets, page_size=20)
    db, qb = open_batch(ctx, prefix, queries)
    assert db.npages == 3
    want, unobserved = null_ref.null_ref(ctx, qb, queries, db, RANDOM_DECOYS, seed=RANDOM_SHUFFLE_SEED, with_unobserved=True)
    yield dict(prefix=prefix, db=db, qb=qb, queries=queries, want=want, unobserved=unobserved)
    qb.close()
    db.close()


def test_random_case_has_teeth(ctx, rnd):
    from priblast_amd import capi
    want = rnd["want"]
    got = capi.search_null(ctx, rnd["qb"], rnd["queries"], rnd["db"], RANDOM_DECOYS, seed=RANDOM_SHUFFLE_SEED)
    assert_bytes(got, want, "random")
    assert ((0 < want["null_le"]) & (want["null_le"] < want["null_hits"])).any()
    assert ((want["null_le"] == 0) & (want["null_hits"] > 0)).any()
    assert (want["null_hits"] == 0).any()
    assert rnd["unobserved"] > 0
    assert len(set(want["page"].tolist())) == 3 and len(set(want["query"].tolist())) == 3
    key = list(zip(want["query"].tolist(), want["page"].tolist(), want["db_id"].tolist()))
    assert key == sorted(key)


# ------------------------------------------------------------------------- 3. a query whose shuffle is forced
def test_forced_shuffle_counts_every_decoy(ctx, tmp_path):
    from priblast_amd import capi
    query = "AC" * 40
    assert capi.shuffle_sequence(query, 9, 0, 4) == query  # (every successor list holds one symbol)
    rng = np.random.default_rng(2)
    pad = lambda n: "".join(rng.choice(list("ACGU"), n))
    targets = [pad(30) + "GU" * k + pad(30) for k in (12, 20, 30)] + [pad(100)]
    prefix = str(tmp_path / "gudb")
    capi.db_build(ctx, prefix, [f"gu{i}" for i in range(len(targets))], targets, page_size=2)
    db, qb = open_batch(ctx, prefix, [query])
    try:
        got = capi.search_null(ctx, qb, [query], db, 4, seed=9)
        assert len(got) >= 3
        assert (got["null_hits"] == 4).all() and (got["null_le"] == 4).all()
        assert got["null_min"].tobytes() == got["e_min"].tobytes()
        assert_bytes(got, null_ref.null_ref(ctx, qb, [query], db, 4, seed=9), "forced")
    finally:
        qb.close()
        db.close()


# ------------------------------------------------------------------------- 4. invariance
def test_same_bytes_with_a_query_per_sub_batch(ctx, mix, monkeypatch):
    """PRB_SEARCH_PAIRS=1 cuts every batch - the real one and the decoys' - into sub-batches of one query: on the golden
    case, whose default run test_mix_equals_the_reference pins (the random case takes 7 s this way)"""
    from priblast_amd import capi
    db, qb, seqs = mix
    want = capi.search_null(ctx, qb, seqs, db, 3, seed=7, file_pos0=2)
    monkeypatch.setenv("PRB_SEARCH_PAIRS", "1")
    for mask in (True, False):
        assert_bytes(capi.search_null(ctx, qb, seqs, db, 3, seed=7, file_pos0=2, mask=mask), want, ("one query per sub-batch", mask))
    assert len(want) > 0


@pytest.mark.parametrize("knob", ["PRB_GAPPED_CHUNK_HITS=3", "one_resident_page", "decoys_one_by_one", "decoy_batches_of_4",
                                  "pages_reversed", "unmasked"])
def test_same_bytes_under(ctx, rnd, monkeypatch, knob):
    from priblast_amd import capi
    kw, db, qb = {}, rnd["db"], rnd["qb"]
    own = None
    if "=" in knob:
        monkeypatch.setenv(*knob.split("="))
    elif knob == "one_resident_page":
        own = open_batch(ctx, rnd["prefix"], rnd["queries"], max_resident_pages=1)
        db, qb = own
    elif knob == "decoys_one_by_one":
        kw["decoy_batch"] = 1
    elif knob == "decoy_batches_of_4":
        kw["decoy_batch"] = 4  # (batches that hold decoys of two queries)
    elif knob == "pages_reversed":
        kw["pages"] = [2, 1, 0]
    elif knob == "unmasked":
        kw["mask"] = False
    try:
        got, counts, dcounts = capi.search_null(ctx, qb, rnd["queries"], db, RANDOM_DECOYS, seed=RANDOM_SHUFFLE_SEED, with_counts=True, **kw)
        assert_bytes(got, rnd["want"], knob)
        if knob == "one_resident_page":
            assert db.page_uploads > 3
        if knob == "unmasked":  # the mask drops seeds: the same table from fewer of them
            _, _, masked = capi.search_null(ctx, qb, rnd["queries"], db, RANDOM_DECOYS, seed=RANDOM_SHUFFLE_SEED, with_counts=True)
            assert 0 < masked[0] < dcounts[0], (masked, dcounts)
            assert masked[2] < dcounts[2]  # (the decoys' unobserved pairs have final hits too)
    finally:
        if own:
            own[1].close()
            own[0].close()


# ------------------------------------------------------------------------- 5. under -u and -j
@pytest.fixture(scope="module")
def planted(ctx, tmp_path_factory):
    """distinct_ref's planted case - pairs with dense runs of intersecting final hits under -f -3 -g -6.5 - in three pages"""
    from priblast_amd import capi
    from distinct_ref import planted_sequences
    _, queries, tnames, targets = planted_sequences()
    prefix = str(tmp_path_factory.mktemp("planted_null") / "pdb")
    capi.db_build(ctx, prefix, tnames, targets, page_size=7)
    db, qb = open_batch(ctx, prefix, queries)
    assert db.npages == 3
    yield db, qb, queries
    qb.close()
    db.close()


@pytest.mark.parametrize("field", ["distinct_sites", "chain_sites"])
def test_thinned_lists(ctx, planted, field):
    from priblast_amd import capi
    db, qb, seqs = planted
    relaxed = dict(interaction_threshold=-3.0, final_threshold=-6.5)
    o = capi.default_opts(**{field: 1}, **relaxed)
    plain = capi.search_null(ctx, qb, seqs, db, 2, seed=7, opts=capi.default_opts(**relaxed))
    got = capi.search_null(ctx, qb, seqs, db, 2, seed=7, opts=o)
    assert_bytes(got, null_ref.null_ref(ctx, qb, seqs, db, 2, seed=7, opts=o), field)
    assert len(got) == len(plain) > 0 and int(got["hits"].sum()) < int(plain["hits"].sum())  # the selection dropped hits
    with capi.NullSet(ctx, qb, db, 3) as ns:  # one selection per table
        ns.observed(0, o)
        with pytest.raises(capi.PrbError, match=field):
            ns.decoys(qb, 0, np.arange(len(seqs)), np.zeros(len(seqs), int), capi.default_opts())


# ------------------------------------------------------------------------- the search entries' own refusals
def test_search_entries_refuse_before_they_search(ctx, mix):
    from priblast_amd import capi
    db, qb, seqs = mix
    n = len(seqs)
    with capi.NullSet(ctx, qb, db, 2) as ns:
        with pytest.raises(capi.PrbError, match="not observed"):
            ns.decoys(qb, 0, np.arange(n), np.zeros(n, int))
        ns.observed(0)
        with pytest.raises(capi.PrbError, match="already observed"):
            ns.observed(0)
        with pytest.raises(capi.PrbError, match="decoy"):
            ns.decoys(qb, 0, np.arange(n), np.full(n, 2))
        with pytest.raises(capi.PrbError, match="owner"):
            ns.decoys(qb, 0, np.arange(n) + 1, np.zeros(n, int))
        with pytest.raises(capi.PrbError, match="twice"):
            ns.decoys(qb, 0, np.zeros(n, int), np.zeros(n, int))
        ns.decoys(qb, 0, np.arange(n), np.zeros(n, int))  # (the queries as their own decoys)
        with pytest.raises(capi.PrbError, match="already merged"):
            ns.decoys(qb, 0, np.arange(n), np.zeros(n, int))
        with pytest.raises(capi.PrbError, match="are merged"):
            ns.finish()
        ns.decoys(qb, 0, np.arange(n), np.ones(n, int))
        for p in range(1, db.npages):
            ns.observed(p)
            for d in range(2):
                ns.decoys(qb, p, np.arange(n), np.full(n, d))
        got = ns.finish()
        assert (got["null_hits"] == 2).all() and (got["null_le"] == 2).all()  # a query is a decoy that ties with itself
        assert got["null_min"].tobytes() == (got["e_min"] + 0.0).tobytes()
        assert ns.decoy_counts()[2] == 2 * ns.counts()[2]
    ms, launches = ctx.stage_ms("null")
    assert launches > 0
