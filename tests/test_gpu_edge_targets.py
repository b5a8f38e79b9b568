"""GPU tests on the `edge` golden case (tests/golden/make_golden.py: edge_inputs; tests/test_edge_targets.py holds what
the fixture guarantees): tiny and adjacent targets, hits flush with both ends of their sequence, trap neighbours
behind the separators, sites at text position 0 and nchars - 1, a page of one sequence.  Every path and every result
table runs over it, each against the yardstick of its own test module."""
import os
import subprocess

import numpy as np
import pytest

import chain_ref
import distinct_ref
import refdump
import test_gpu_coverage as cov
import test_gpu_profile as prof
import test_gpu_targets as tgt
import test_gpu_top as top
from test_gpu_cli import body
from test_gpu_distinct import assert_pages, search
from test_gpu_options import OPTION_SETS, ORACLE_NAMES
from test_gpu_search import SEED_PATHS, as_dicts, key, same
from test_gpu_summary import assert_same, reduce_hits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAGE = 8  # db -c of the case


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge")
    refdump.unpack_case(GOLDEN, "edge", str(d))
    return str(d)


@pytest.fixture(scope="module")
def edge(ctx, edge_dir):
    """the edge database (resident), its queries as one batch, and the default path's result per stage and page"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_q.fa"))
    db = capi.Db(ctx, os.path.join(edge_dir, "edgedb"))
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)

    class Edge:
        pass
    e = Edge()
    e.names, e.seqs, e.db, e.qb, e.prefix = names, seqs, db, qb, os.path.join(edge_dir, "edgedb")
    e.ids = np.arange(len(seqs), dtype=np.int32)
    e.default = {stage: run_pages(ctx, qb, db, stage) for stage in (1, 2, 3)}
    yield e
    qb.close()
    db.close()


def run_pages(ctx, qb, db, stage=3, opts=None):
    """[(hits, bp, counts)] per page, copies"""
    from priblast_amd import capi
    out = []
    for p in range(db.npages):
        hits, bp, counts = capi.search_page(ctx, qb, db, p, opts or capi.default_opts(output_style=1), stage)
        out.append((np.array(hits), np.array(bp), tuple(counts)))
    return out


def assert_same_pages(got, want, what):
    assert len(got) == len(want), what
    for p, ((h1, b1, c1), (h2, b2, c2)) in enumerate(zip(got, want)):
        assert c1 == c2, (what, p, c1, c2)
        assert np.array_equal(h1, h2) and np.array_equal(b1, b2), (what, p)


def test_db_build_matches_reference_files(ctx, edge_dir, tmp_path):
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_db.fa"))
    out = str(tmp_path / "edgedb")
    capi.db_build(ctx, out, names, seqs, 0, 8, 70, 5, PAGE)
    for ext in ("bas", "seq", "acc", "nam", "ind"):
        with open(f"{out}.{ext}", "rb") as f, open(os.path.join(edge_dir, f"edgedb.{ext}"), "rb") as g:
            assert f.read() == g.read(), ext


def test_stage_dumps(edge, edge_dir):
    """test_gpu_search.py::test_stage_dumps on the edge case: seeds in emission order, the ungapped split to 1e-12,
    gapped hits and base pairs exact."""
    stg = refdump.read_stages(os.path.join(edge_dir, "edge.stg"))
    assert edge.db.npages == 5
    n = [0, 0, 0]
    for page in range(edge.db.npages):
        per_stage = {s: as_dicts(*edge.default[s][page][:2]) for s in (1, 2, 3)}
        for rec in stg:
            if rec["page"] != page:
                continue
            q = rec["q"]
            mine = {s: [h for h in per_stage[s] if h["query"] == q] for s in (1, 2, 3)}
            assert len(mine[1]) == len(rec["seed"]), (q, page)
            for a, b in zip(mine[1], rec["seed"]):
                assert same(a, b, with_bp=False), (q, page, a, b)
            for s, ref, tol in ((2, rec["ungapped"], 1e-12), (3, rec["gapped"], 0.0)):
                assert len(mine[s]) == len(ref), (q, page, s)
                for a, b in zip(sorted(mine[s], key=key), sorted(ref, key=key)):
                    assert same(a, b, tol), (q, page, s, a, b)
            for s in (1, 2, 3):
                n[s - 1] += len(mine[s])
    assert min(n) > 0


@pytest.mark.parametrize("batch", [None, "1"])
@pytest.mark.parametrize("style", [0, 1])
def test_ris_cli_matches_reference(edge_dir, tmp_path, style, batch):
    from priblast_amd import capi
    out = str(tmp_path / "out.txt")
    env = dict(os.environ)
    env.pop("PRB_BATCH", None)
    if batch:
        env["PRB_BATCH"] = batch
    subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "edge_q.fa"), "-o", out, "-d",
                    os.path.join(edge_dir, "edgedb"), "-s", str(style)], check=True, env=env)
    head, lines = body(out)
    with open(os.path.join(GOLDEN, f"edge_ris_s{style}.out")) as f:
        gold = f.read().splitlines()
    assert head[0] == gold[0] and head[2] == gold[1]
    assert lines == gold[2:]


ALL_STAGES = (1, 2, 3)
PATHS = [(f"{name}{'+chunks' if chunk else ''}", dict(env, **({"PRB_SEARCH_CHUNK_PAIRS": "7"} if chunk else {})), ALL_STAGES)
         for name, env in SEED_PATHS.items() for chunk in (False, True)]
PATHS += [(e, dict(s.partition("=")[::2] for s in e.split(",")), stages) for e, stages in [
    ("PRB_SEARCH_PAIRS=1", ALL_STAGES), ("PRB_GAPPED_FIRST_TIER=1", (3,)), ("PRB_GAPPED_FIRST_TIER=2", (3,)),
    ("PRB_GAPPED_FIRST_TIER=3", (3,)), ("PRB_GAPPED_FIRST_TIER=4", (3,)), ("PRB_GAPPED_FIRST_TIER=4,PRB_GAPPED_WAVE_HBM=1", (3,)),
    ("PRB_GAPPED_FRONT=0", (3,)), ("PRB_GAPPED_FRONT_PAIRED", (3,)), ("PRB_GAPPED_HANDOVER=0", (3,)), ("PRB_GAPPED_PAIR=0", (3,)),
    ("PRB_GAPPED_POOL=0", (3,)), ("PRB_GAPPED_CHUNK_HITS=3", (3,)), ("PRB_TRACE_NO_SLOTS", (3,)), ("PRB_TRACE_SLOT_CAP=1", (3,)),
    ("PRB_FILTER_TILES=0", (3,)), ("PRB_SORT_FOUR_KEYS", (3,))]]


@pytest.mark.parametrize("name,env,stages", PATHS, ids=[p[0] for p in PATHS])
def test_every_path_matches_the_default(ctx, edge, monkeypatch, name, env, stages):
    """hits, base pairs and counts bit-identical to the default path, whatever form the seed part takes, however the
    search is cut up, whichever gapped kernel extends the hits"""
    for k, v in env.items():
        monkeypatch.setenv(k, v or "1")
    for stage in stages:
        assert_same_pages(run_pages(ctx, edge.qb, edge.db, stage), edge.default[stage], (name, stage))


def test_one_resident_page(ctx, edge):
    """every page, the one of a single sequence included, streamed in and out of one slot, forward and backward"""
    from priblast_amd import capi
    db = capi.Db(ctx, edge.prefix, 1)
    try:
        assert_same_pages(run_pages(ctx, edge.qb, db), edge.default[3], "resident=1")
        for p in reversed(range(db.npages)):
            hits, bp, counts = capi.search_page(ctx, edge.qb, db, p, capi.default_opts(output_style=1))
            assert_same_pages([(np.array(hits), np.array(bp), tuple(counts))], [edge.default[3][p]], ("resident=1", p))
    finally:
        db.close()


def rel(bp):
    """a hit's pairs relative to its first ones, as a sorted tuple (hit 0 of a list keeps its pairs unsorted)"""
    return tuple(sorted(map(tuple, (bp - bp.min(axis=0)).tolist())))


def against_oracle(ctx, oracle, prefix, seqs, kw, db=None, qb=None):
    """final hits of every (query, page) against the restatement's: everything exact; -> number of hits"""
    from priblast_amd import capi
    own = db is None
    if own:
        db = capi.Db(ctx, prefix)
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
    odb = oracle.Db(prefix)
    oopts = oracle.default_opts(**{ORACLE_NAMES[k]: v for k, v in kw.items()})
    total = 0
    try:
        for page, (hits, bp, _) in enumerate(run_pages(ctx, qb, db, 3, capi.default_opts(output_style=1, **kw))):
            mine = as_dicts(hits, bp)
            for q, s in enumerate(seqs):
                _, _, gap = odb.stages(s, page, oopts)
                got = [h for h in mine if h["query"] == q]
                assert len(got) == len(gap), (kw, page, q)
                for a, b in zip(sorted(got, key=key), sorted(gap, key=key)):
                    assert same(a, b), (kw, page, q, a, b)
                total += len(got)
    finally:
        odb.close()
        if own:
            qb.close()
            db.close()
    return total


@pytest.mark.parametrize("kw", OPTION_SETS)
def test_option_sweep_matches_oracle(ctx, oracle, edge, kw):
    """-m 1 / -m 9 look ahead, -y 12 / -x 30 drop out, across the separators"""
    assert against_oracle(ctx, oracle, edge.prefix, edge.seqs, kw, edge.db, edge.qb) > 0


def test_targets_below_four_nt_are_loaded_and_never_hit(ctx, oracle, edge, tmp_path):
    """A target of 1, 2 or 3 nt gets L - 4 < 0 as its count of accessibilities in .acc; the reference's `ris` aborts when
    it loads such a database.  Here, HIP path and restatement alike, the count reads as 0: the database
    loads, such a target is never hit, and its neighbours' hits are what they are without it."""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_db.fa"))
    extra = {0: "G", 3: "CG", 8: "GCA", 17: "U", len(seqs): "AGC"}  # in front of these targets / at the very end
    n2, s2 = [], []
    for i in range(len(seqs) + 1):
        if i in extra:
            n2.append(f"short_before_{i}")
            s2.append(extra[i])
        if i < len(seqs):
            n2.append(names[i])
            s2.append(seqs[i])
    prefix = str(tmp_path / "shortdb")
    capi.db_build(ctx, prefix, n2, s2, 0, 8, 70, 5, PAGE)
    counts = [n for n, _, _, _ in refdump.read_acc(prefix + ".acc", len(s2))]
    assert min(counts) == -3 and counts == [len(s) - 4 for s in s2]
    assert against_oracle(ctx, oracle, prefix, edge.seqs, {}) > 0
    db = capi.Db(ctx, prefix)
    try:
        mine = sorted((edge.names[h["query"]], n2[p * PAGE + h["db_id"]], h["e_tot"], h["db_len"], rel(h["bp"]))
                      for p, (hits, bp, _) in enumerate(run_pages(ctx, edge.qb, db)) for h in as_dicts(hits, bp))
    finally:
        db.close()
    dnames, _ = refdump.read_fasta(os.path.join(GOLDEN, "edge_db.fa"))
    plain = sorted((edge.names[h["query"]], dnames[p * PAGE + h["db_id"]], h["e_tot"], h["db_len"], rel(h["bp"]))
                   for p, (hits, bp, _) in enumerate(edge.default[3]) for h in as_dicts(hits, bp))
    assert mine == plain


def test_summary_top_and_targets(ctx, edge):
    from priblast_amd import capi
    opts = capi.default_opts(output_style=0)
    pages = []
    for p in range(edge.db.npages):
        hits, bp, counts = capi.search_page(ctx, edge.qb, edge.db, p, opts)
        ref = reduce_hits(hits, bp)
        pairs, pcounts = capi.search_page_summary(ctx, edge.qb, edge.db, p, opts, with_counts=True)
        assert tuple(pcounts) == tuple(counts)
        assert_same(pairs, ref, ("edge", p))
        pages.append((np.array(pairs), pcounts))
    recs = [r for r, _ in pages]
    assert sum(len(r) for r in recs) > 10
    sums = tuple(int(sum(c[i] for _, c in pages)) for i in range(3))
    most = int(np.bincount(np.concatenate(recs)["query"]).max())
    for n in (1, 2, most + 5):
        got, counts = capi.search_top(ctx, edge.qb, edge.db, n, opts, with_counts=True)
        assert counts == sums
        top.assert_bytes(got, top.rank(recs, n), ("top", n))
    calls = [(edge.ids, p, r) for p, r in enumerate(recs)]
    most = tgt.most_per_target(calls)
    assert most >= 2
    for n in (1, 2, most + 5):
        got, counts = capi.search_targets(ctx, edge.db, n, [(edge.qb, edge.ids)], opts, with_counts=True)
        assert counts == sums
        tgt.assert_bytes(got, tgt.rank(calls, n), ("targets", n))


def test_profile(ctx, edge):
    from priblast_amd import capi
    pages, counts = prof.hit_path(ctx, edge.qb, edge.db)
    got, got_counts = capi.search_profile(ctx, edge.qb, edge.db, with_counts=True)
    assert got_counts == counts
    want = prof.profile(pages, [len(s) for s in edge.seqs])
    assert len(want) > 0
    prof.assert_bytes(got, want, "edge")


def test_coverage(ctx, edge):
    """regions at depth 1 and 2 against the numpy table; no region leaves its sequence, and two targets next to each
    other in the text (a span that ends at a sequence's last base puts its -1 into the separator's slot) keep their
    own regions"""
    from priblast_amd import capi
    info = cov.seq_info(edge.db)
    calls, counts = cov.hit_calls(ctx, edge.qb, edge.db, edge.ids)
    tab = cov.table(calls, info)
    assert cov.max_depth(tab) >= 2
    for d in (1, 2):
        got, got_counts = capi.search_coverage(ctx, edge.db, d, [(edge.qb, edge.ids)], with_counts=True)
        assert got_counts == counts
        want = cov.regions(tab, info, d)
        assert len(want) > 0
        tgt.assert_bytes(got, want, ("coverage", d))
        for r in got:
            L = info[int(r["page"])][int(r["db_id"])][0]
            assert 0 <= r["start"] <= r["end"] < L, r
        if d == 1:
            owners = {(int(r["page"]), int(r["db_id"])) for r in got}
            assert owners == set(tab)  # every target with a hit has a region of its own
            adjacent = [(p, i) for (p, i) in owners if (p, i + 1) in owners]
            assert adjacent
            whole = [(p, i) for (p, i) in owners if any(r["page"] == p and r["db_id"] == i and r["start"] == 0 and
                                                        r["end"] == info[p][i][0] - 1 for r in got)]
            assert whole  # a region from a sequence's first base to its last


@pytest.mark.parametrize("mode,ref", [("distinct_sites", distinct_ref), ("chain_sites", chain_ref)])
def test_distinct_and_chain_sites(ctx, edge, mode, ref):
    from priblast_amd import capi
    for style in (0, 1):
        plain = search(ctx, edge.qb, edge.db, capi.default_opts(output_style=style))
        want = [ref.filter_page(h, bp)[:2] + (c,) for h, bp, c in plain]
        got = search(ctx, edge.qb, edge.db, capi.default_opts(output_style=style, **{mode: 1}))
        assert_pages(got, want, (mode, style))
        assert sum(len(w[0]) for w in want) > 0
