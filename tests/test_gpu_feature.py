"""GPU tests of the feature table on the search path (prb_search_page_features) through the C ABI, on the `mix` and `edge`
fixtures.  The yardstick is tests/feature_ref.py's fold of the hits that prb_search_page(..., 3) returns with the same
options; the annotation is the one test_feature_host.py checks against the golden hits.  Records must match byte for byte."""
import os

import numpy as np
import pytest

import feature_ref
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


def hit_pages(ctx, qb, db, opts=None):
    from priblast_amd import capi
    out, counts = {}, [0, 0, 0]
    for p in range(db.npages):
        hits, bp, c = capi.search_page(ctx, qb, db, p, opts or capi.default_opts())
        out[p] = (hits, bp)
        counts = [a + b for a, b in zip(counts, c)]
    return out, tuple(counts)


def load(ctx, golden_dir, tag):
    """the fixture `tag`: database, batch, the golden annotation as (page, db_id, start, end), the sequences' (start_pos,
    length), and the plain search's hits - the reference's input, computed once and never changed"""
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
    with open(os.path.join(GOLDEN, f"{tag}_ris_s1.out")) as f:
        named = feature_ref.golden_annotation(f.read().splitlines()[2:])
    where, seq_of = {}, []
    for p in range(db.npages):
        seq_of.append([])
        for i in range(db.page_info(p)[0]):
            where.setdefault(db.seq_name(p, i), (p, i))
            length, _, start_pos = db.seq_lengths(p, i)
            seq_of[p].append((start_pos, length))
    annot = [where[t] + (s, e) for t, s, e, _ in named]
    hits, counts = hit_pages(ctx, qb, db)
    return dict(db=db, qb=qb, seqs=seqs, annot=annot, seq_of=seq_of, hits=hits, counts=counts, prefix=os.path.join(golden_dir, f"{tag}db"))


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    c = load(ctx, golden_dir, "mix")
    assert c["db"].npages == 3
    yield c
    c["qb"].close()
    c["db"].close()


@pytest.fixture(scope="module")
def edge(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("feature_edge")
    refdump.unpack_case(GOLDEN, "edge", str(d))
    c = load(ctx, str(d), "edge")
    yield c
    c["qb"].close()
    c["db"].close()


def table(ctx, c, opts=None, pages=None, db=None, qb=None):
    from priblast_amd import capi
    db, qb = db or c["db"], qb or c["qb"]
    with capi.Annotation(ctx, db, c["annot"]) as an:
        return capi.search_features(ctx, qb, db, an, opts, pages, with_counts=True)


@pytest.mark.parametrize("tag", ["mix", "edge"])
def test_features_equal_the_reference_fold_of_the_hits(ctx, mix, edge, tag):
    c = mix if tag == "mix" else edge
    got, un, counts = table(ctx, c)
    want, want_un = feature_ref.fold(c["hits"], c["annot"], c["seq_of"])
    assert got.tobytes() == want.tobytes(), (got, want)
    assert un == want_un and len(got) >= 5 and un > 0
    assert counts == c["counts"]
    final = sum(len(h) for h, _ in c["hits"].values())
    assert counts[2] == final and int(got["hits"].sum()) >= final - un
    assert (got["inside"] < got["hits"]).any() and (got["inside"] > 0).any()


def test_selections_and_a_pair_mask(ctx, mix):
    from priblast_amd import capi
    c = mix
    for kw in (dict(distinct_sites=1), dict(chain_sites=1)):
        o = capi.default_opts(**kw)
        want, want_un = feature_ref.fold(hit_pages(ctx, c["qb"], c["db"], o)[0], c["annot"], c["seq_of"])
        got, un, _ = table(ctx, c, o)
        assert got.tobytes() == want.tobytes() and un == want_un and len(got) > 2, kw
    pairs = sorted({(int(h["query"]), p, int(h["db_id"])) for p, (hits, _) in c["hits"].items() for h in hits})
    annotated = {(p, d) for p, d, _, _ in c["annot"]}
    allowed = [x for x in pairs if (x[1], x[2]) in annotated] + [x for x in pairs if (x[1], x[2]) not in annotated][::2]
    pm = capi.PairMask(ctx, c["qb"], c["db"])
    try:
        pm.allow(*[np.array([a[k] for a in allowed], np.int32) for k in range(3)])
        o = capi.default_opts()
        o.allowed_pairs = pm.h.value
        want, want_un = feature_ref.fold(hit_pages(ctx, c["qb"], c["db"], o)[0], c["annot"], c["seq_of"])
        got, un, _ = table(ctx, c, o)
        assert got.tobytes() == want.tobytes() and un == want_un and len(got) > 2
        assert un < feature_ref.fold(c["hits"], c["annot"], c["seq_of"])[1]
    finally:
        pm.close()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "resident=1", "pages=2,0,1"])
def test_feature_invariance(ctx, mix, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; the 3-page database streamed through one resident
    page; the pages in another order: the same bytes"""
    c = mix
    name, value = knob.split("=")
    if name not in ("resident", "pages"):
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, c["prefix"], c["seqs"], int(value) if name == "resident" else None)
    try:
        pages = [int(p) for p in value.split(",")] if name == "pages" else None
        got, un, _ = table(ctx, c, pages=pages, db=db, qb=qb)
        want, want_un = feature_ref.fold(c["hits"], c["annot"], c["seq_of"])
        assert got.tobytes() == want.tobytes() and un == want_un, knob
    finally:
        qb.close()
        db.close()


def test_two_contexts_share_the_pages_and_merge(mix):
    from priblast_amd import capi
    c = mix
    want, want_un = feature_ref.fold(c["hits"], c["annot"], c["seq_of"])
    ctxs = [capi.Context(0), capi.Context(0)]
    opened = [open_batch(x, c["prefix"], c["seqs"]) for x in ctxs]
    try:
        annots = [capi.Annotation(x, db, c["annot"]) for x, (db, _) in zip(ctxs, opened)]
        tables = [capi.FeatSet(x, qb, an) for x, (_, qb), an in zip(ctxs, opened, annots)]
        tables[1].merge(opened[1][0], 2)
        tables[0].merge(opened[0][0], 1)
        tables[1].merge(opened[1][0], 0)
        tables[0].absorb(tables[1])
        assert tables[1].unassigned() == 0
        got = tables[0].finish()
        assert got.tobytes() == want.tobytes() and tables[0].unassigned() == want_un
        assert tables[0].counts() == c["counts"]
        with pytest.raises(capi.PrbError, match="finished"):
            tables[0].absorb(tables[1])
        assert len(tables[1].finish()) == 0
        for t in tables:
            t.close()
        for an in annots:
            an.close()
    finally:
        for (db, qb), x in zip(opened, ctxs):
            qb.close()
            db.close()
            x.close()


def test_the_table_guards(ctx, mix):
    from priblast_amd import capi
    c = mix
    db, qb = c["db"], c["qb"]
    other = capi.QBatch(ctx, c["seqs"][:2], db.repeat_flag)
    other.accessibility(db.W, db.delta)
    try:
        with capi.Annotation(ctx, db, c["annot"]) as an, capi.FeatSet(ctx, qb, an) as fs:
            fs.merge(db, 0)
            with pytest.raises(capi.PrbError, match="page 0 is already merged"):
                fs.merge(db, 0)
            with pytest.raises(capi.PrbError, match="distinct_sites"):
                fs.merge(db, 1, capi.default_opts(distinct_sites=1))
            with pytest.raises(capi.PrbError, match="chain_sites"):
                fs.merge(db, 1, capi.default_opts(chain_sites=1))
            with pytest.raises(capi.PrbError, match="another context or query batch"):
                fs.merge(db, 1, qb=other)
            fs.add_hits(1, *c["hits"][1])  # a caller's hits and searched pages in one table
            fs.merge(db, 2)
            want, want_un = feature_ref.fold(c["hits"], c["annot"], c["seq_of"])
            assert fs.finish().tobytes() == want.tobytes() and fs.unassigned() == want_un
    finally:
        other.close()
