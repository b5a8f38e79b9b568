"""GPU tests of the group table on the search path (prb_search_page_groups) through the C ABI, on the `mix` fixture: its
database has 3 pages, so groups span pages.  The yardstick is tests/group_ref.py's fold of capi.search_page_summary's
records - pinned to the hit path by test_gpu_summary.py.  The table must match it byte for byte."""
import os

import numpy as np
import pytest

import group_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


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


def group_maps(db, per_group):
    """consecutive targets of the whole database, `per_group` to a group (so groups span the pages' borders)"""
    maps, t = [], 0
    for p in range(db.npages):
        nseq = db.page_info(p)[0]
        maps.append([(t + i) // per_group for i in range(nseq)])
        t += nseq
    return maps, (t + per_group - 1) // per_group


def summaries(ctx, qb, db, opts):
    from priblast_amd import capi
    return {p: capi.search_page_summary(ctx, qb, db, p, opts) for p in range(db.npages)}


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, "mixdb"), seqs)
    assert db.npages == 3
    maps, ng = group_maps(db, 4)
    assert any(maps[p][-1] == maps[p + 1][0] for p in range(2))  # a group spans two pages
    recs = summaries(ctx, qb, db, capi.default_opts())  # the reference's input: computed once, never changed
    assert sum(len(r) for r in recs.values()) > 10
    yield db, qb, seqs, maps, ng, recs
    qb.close()
    db.close()


def test_groups_equal_the_reference_fold_of_the_summaries(ctx, mix):
    from priblast_amd import capi
    db, qb, _, maps, ng, recs = mix
    for n in (0, 1, 3):
        got, counts = capi.search_groups(ctx, qb, db, maps, ng, n, with_counts=True)
        want = group_ref.fold(recs, maps, ng, n)
        assert got.tobytes() == want.tobytes(), (n, got, want)
        assert counts[2] == sum(int(r["hits"]) for p in recs for r in recs[p])
    got = capi.search_groups(ctx, qb, db, maps, ng)
    assert (got["members"] > 1).any() and int(got["group_hits"].sum()) == sum(int(r["hits"]) for p in recs for r in recs[p])
    assert int(got["members"].sum()) == sum(len(r) for r in recs.values())


def test_the_identity_map_gives_the_summary_records(ctx, mix):
    from priblast_amd import capi
    db, qb, _, _, _, recs = mix
    maps, ng = group_maps(db, 1)
    got = capi.search_groups(ctx, qb, db, maps, ng)
    want = sorted(((int(r["query"]), p, int(r["db_id"])), r) for p in recs for r in recs[p])
    assert len(got) == len(want)
    for g, (key, r) in zip(got, want):
        assert (int(g["query"]), int(g["page"]), int(g["db_id"])) == key
        assert g.tobytes()[:capi.PAIR_DTYPE.itemsize] == r.tobytes()
        assert int(g["members"]) == 1 and int(g["group_hits"]) == int(r["hits"]) and int(g["rank"]) == 0


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "resident=1", "pages=2,0,1"])
def test_group_invariance(ctx, golden_dir, mix, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; the 3-page database streamed through one resident
    page; the pages in another order: the same bytes"""
    from priblast_amd import capi
    _, _, seqs, maps, ng, recs = mix
    name, value = knob.split("=")
    if name not in ("resident", "pages"):
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, os.path.join(golden_dir, "mixdb"), seqs, int(value) if name == "resident" else None)
    try:
        pages = [int(p) for p in value.split(",")] if name == "pages" else None
        for n in (0, 2):
            assert capi.search_groups(ctx, qb, db, maps, ng, n, pages=pages).tobytes() == group_ref.fold(recs, maps, ng, n).tobytes(), (knob, n)
    finally:
        qb.close()
        db.close()


def test_groups_of_the_distinct_sites_and_under_a_pair_mask(ctx, mix):
    from priblast_amd import capi
    db, qb, _, maps, ng, recs = mix
    o = capi.default_opts(distinct_sites=1)
    want = group_ref.fold(summaries(ctx, qb, db, o), maps, ng)
    got = capi.search_groups(ctx, qb, db, maps, ng, opts=o)
    assert got.tobytes() == want.tobytes() and len(got) > 3
    # a mask that allows every second observed pair
    allowed = [(int(r["query"]), p, int(r["db_id"])) for p in recs for r in recs[p]][::2]
    pm = capi.PairMask(ctx, qb, db)
    try:
        pm.allow(np.array([a[0] for a in allowed], np.int32), np.array([a[1] for a in allowed], np.int32), np.array([a[2] for a in allowed], np.int32))
        o = capi.default_opts()
        o.allowed_pairs = pm.h.value
        want = group_ref.fold(summaries(ctx, qb, db, o), maps, ng, 2)
        got = capi.search_groups(ctx, qb, db, maps, ng, 2, opts=o)
        assert got.tobytes() == want.tobytes() and 0 < int(got["members"].sum()) <= len(allowed)
    finally:
        pm.close()


def test_a_page_is_merged_once_and_for_its_own_table(ctx, mix):
    from priblast_amd import capi
    db, qb, seqs, maps, ng, recs = mix
    with capi.GroupSet(ctx, qb, db, maps, ng) as gs:
        gs.merge(0)
        with pytest.raises(capi.PrbError, match="page 0 is already merged"):
            gs.merge(0)
        with pytest.raises(capi.PrbError, match="distinct_sites"):
            gs.merge(1, capi.default_opts(distinct_sites=1))
        gs.add_pairs(1, recs[1])  # a caller's records and a searched page in one table
        gs.merge(2)
        assert gs.finish().tobytes() == group_ref.fold(recs, maps, ng).tobytes()
