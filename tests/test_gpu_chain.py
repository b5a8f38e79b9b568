"""GPU tests of opts.chain_sites (`ris -j`) through the search.  The yardstick is the plain hit path - prb_search_page
with chain_sites = 0, pinned to the reference by test_gpu_search.py / test_gpu_options.py - filtered in Python by the
rule of include/priblast_hip.h (chain_ref.filter_page); the other modes are compared with the existing Python
restatements of their contracts over those filtered hits."""
import os

import numpy as np
import pytest

import distinct_ref
import refdump
import test_gpu_coverage as cov
import test_gpu_targets as tgt
from chain_ref import chain_of_each_run, filter_page
from distinct_ref import planted_sequences
from test_gpu_distinct import OPTS, RELAXED, assert_pages, pair_records, search
from test_gpu_profile import profile
from test_gpu_summary import assert_same, bits, reduce_hits
from test_gpu_top import rank
from test_gpu_tophits import Ranking, assert_bytes, open_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def filtered(plain):
    """the yardstick: [(hits, bp, counts of the plain search)] per page"""
    return [filter_page(h, bp)[:2] + (c,) for h, bp, c in plain]


def test_goldens(ctx, golden_dir):
    """every kept record is a record of the plain result, and the kept ones are chain_ref's"""
    from priblast_amd import capi
    dropped = 0
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
        try:
            for kw in OPTS:
                for style in (0, 1):
                    plain = search(ctx, qb, db, capi.default_opts(output_style=style, **kw))
                    want = filtered(plain)
                    got = search(ctx, qb, db, capi.default_opts(output_style=style, chain_sites=1, **kw))
                    assert_pages(got, want, (tag, kw, style))
                    dropped += sum(len(p[0]) for p in plain) - sum(len(w[0]) for w in want)
        finally:
            qb.close()
            db.close()
    print("hits dropped over the goldens:", dropped)
    assert dropped > 0


@pytest.fixture(scope="module")
def planted(ctx, tmp_path_factory):
    """the planted case (distinct_ref.planted_sequences) as a database of three pages, its plain hits for both output
    styles and what the rule keeps of them - computed once, never changed"""
    from priblast_amd import capi
    qnames, queries, tnames, targets = planted_sequences()
    prefix = str(tmp_path_factory.mktemp("planted_chain") / "pdb")
    capi.db_build(ctx, prefix, tnames, targets, page_size=7)
    db, qb = open_batch(ctx, prefix, queries)
    try:
        assert db.npages == 3
        plain = {style: search(ctx, qb, db, capi.default_opts(output_style=style, **RELAXED)) for style in (0, 1)}
    finally:
        qb.close()
        db.close()
    return dict(prefix=prefix, qnames=qnames, queries=queries, tnames=tnames, plain=plain, want={s: filtered(p) for s, p in plain.items()})


def test_planted_case_has_chains(planted):
    """what the other tests lean on, on the PLAIN output: without it a library that ignored the option, or ran the -u
    selection in its place, could pass.  (On the reference's output: 501 hits in 34 pairs, 69 kept, chains of two to
    five hits in 19 pairs, the chain differs from the distinct sites in 24 pairs.)"""
    total, kept, chain_len, lengths, differs = 0, 0, [], [], 0
    for hits, _, _ in planted["plain"][0]:
        greedy = distinct_ref.keep_mask(hits)
        for a, b, members, _ in chain_of_each_run(hits):
            chain_len.append(len(members))
            lengths.append(b - a)
            keep = np.zeros(b - a, bool)
            keep[members - a] = True
            differs += int((keep != greedy[a:b]).any())
        total += len(hits)
    kept = sum(chain_len)
    print("planted case: hits", total, "kept", kept, "pairs", len(chain_len), "chains of two or more", sum(c >= 2 for c in chain_len),
          "longest chain", max(chain_len), "longest run", max(lengths), "pairs where -u differs", differs)
    assert max(lengths) > 64
    assert sum(c >= 2 for c in chain_len) >= 1
    assert differs >= 1
    assert kept < total


KNOBS = ["plain", "PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=37", "resident=1", "PRB_CHAIN_LDS_HITS=1", "PRB_CHAIN_LDS_HITS=40"]


@pytest.mark.parametrize("knob", KNOBS)
def test_planted_hits_and_invariance(ctx, planted, monkeypatch, knob):
    """the kept hits, byte for byte, for both output styles - whatever cuts the batch, chunks the gapped stage, streams
    the pages or moves the selection's scores to HBM"""
    from priblast_amd import capi
    name, _, value = knob.partition("=")
    if name.startswith("PRB_"):
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"], int(value) if name == "resident" else None)
    try:
        for style in (0, 1):
            ctx.reset_timers()
            got = search(ctx, qb, db, capi.default_opts(output_style=style, chain_sites=1, **RELAXED))
            assert_pages(got, planted["want"][style], (knob, style))
            assert sum(len(g[0]) for g in got) < sum(g[2][2] for g in got)  # size below counts[2]: hits were dropped
            assert ctx.stage_ms("chain")[1] > 0 and ctx.stage_ms("distinct") == (0.0, 0)
        if name == "plain":  # the timer stays silent without the option
            ctx.reset_timers()
            search(ctx, qb, db, capi.default_opts(**RELAXED))
            assert ctx.stage_ms("chain") == (0.0, 0)
            # last_stage 1 and 2 ignore the field
            for stage in (1, 2):
                a = capi.search_page(ctx, qb, db, 0, capi.default_opts(chain_sites=1, **RELAXED), stage)
                b = capi.search_page(ctx, qb, db, 0, capi.default_opts(**RELAXED), stage)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
            assert ctx.stage_ms("chain") == (0.0, 0)
    finally:
        qb.close()
        db.close()


def test_planted_summary_is_the_chain(ctx, planted):
    """-t over the kept hits: hits = the chain's length, e_sum = its score S bit for bit, the best hit = its
    lowest-energy member"""
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    on = capi.default_opts(output_style=0, chain_sites=1, **RELAXED)
    try:
        longer = 0
        for p in range(db.npages):
            hits, bp, plain_counts = planted["plain"][0][p]
            pairs, c = capi.search_page_summary(ctx, qb, db, p, on, with_counts=True)
            assert tuple(c) == tuple(plain_counts)
            runs = chain_of_each_run(hits)
            assert len(pairs) == len(runs)
            for rec, (a, b, members, score) in zip(pairs, runs):
                assert (int(rec["query"]), int(rec["db_id"])) == (int(hits["query"][a]), int(hits["db_id"][a]))
                assert int(rec["hits"]) == len(members)
                assert bits(rec["e_sum"]) == bits(score), (p, a, float(rec["e_sum"]), score)
                best = members[np.argmin(hits["e_tot"][members])]  # (argmin: the first of equals)
                assert bits(rec["e_min"]) == bits(hits["e_tot"][best])
                assert rec["bp_first"].tolist() == bp[hits["bp_offset"][best]].tolist()
                assert rec["bp_last"].tolist() == bp[hits["bp_offset"][best] + 1].tolist()
                longer += len(members) >= 2
            want = planted["want"][0][p]
            assert_same(pairs, reduce_hits(want[0], want[1]), ("summary", p))
        assert longer > 0
    finally:
        qb.close()
        db.close()


def test_planted_tables(ctx, planted):
    """all five tables, every page merged = their restatements over the filtered hits"""
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    want0, want1 = planted["want"][0], planted["want"][1]
    counts = tuple(int(sum(w[2][i] for w in want0)) for i in range(3))
    ids = np.arange(len(planted["queries"]), dtype=np.int32)
    try:
        on0 = capi.default_opts(output_style=0, chain_sites=1, **RELAXED)
        on1 = capi.default_opts(output_style=1, chain_sites=1, **RELAXED)
        pair_pages = [pair_records(h, bp) for h, bp, _ in want0]
        for n in (1, 3):
            recs, c = capi.search_top(ctx, qb, db, n, on0, with_counts=True)
            want = rank(pair_pages, n)
            assert recs.tobytes() == want.tobytes() and c == counts, ("top", n)
        for opts, want in ((on0, want0), (on1, want1)):
            ranking = Ranking([(h, bp) for h, bp, _ in want])
            for n in (1, 5, 64):
                recs, bp, c = capi.search_tophits(ctx, qb, db, n, opts, with_counts=True)
                assert_bytes((recs, bp), ranking.cut(n), ("tophits", opts.output_style, n))
                assert c == counts
        rows, c = capi.search_profile(ctx, qb, db, on0, with_counts=True)
        pages = []
        for p, (h, bp, _) in enumerate(want0):
            off = h["bp_offset"].astype(np.int64)
            pages.append((p, h, bp[off], bp[off + 1]))
        want = profile(pages, [len(q) for q in planted["queries"]])
        assert rows.tobytes() == want.tobytes() and c == counts
        # the target table and the coverage table
        calls = [(ids, p, recs) for p, recs in enumerate(pair_pages)]
        for n in (1, 2):
            got, c = capi.search_targets(ctx, db, n, [(qb, ids)], on0, with_counts=True)
            tgt.assert_bytes(got, tgt.rank(calls, n), ("targets", n))
            assert c == counts
        info = cov.seq_info(db)
        tab = cov.table([(ids, p, h, bp) for p, (h, bp, _) in enumerate(want0)], info)
        for d in (1, 2):
            got, c = capi.search_coverage(ctx, db, d, [(qb, ids)], on0, with_counts=True)
            tgt.assert_bytes(got, cov.regions(tab, info, d), ("coverage", d))
            assert c == counts
    finally:
        qb.close()
        db.close()


def test_option_refusals(ctx, planted):
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    try:
        for bad in (2, -1):
            with pytest.raises(capi.PrbError, match="chain_sites"):
                capi.search_page(ctx, qb, db, 0, capi.default_opts(chain_sites=bad))
            with pytest.raises(capi.PrbError, match="chain_sites"):
                capi.search_page_summary(ctx, qb, db, 0, capi.default_opts(chain_sites=bad))
        with pytest.raises(capi.PrbError, match="chain_sites and distinct_sites"):
            capi.search_page(ctx, qb, db, 0, capi.default_opts(chain_sites=1, distinct_sites=1))
        assert capi.default_opts().chain_sites == 0
    finally:
        qb.close()
        db.close()


@pytest.mark.parametrize("kind", ["top", "tophits", "profile", "targets", "coverage"])
def test_a_table_holds_pages_of_one_value(ctx, planted, kind):
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    off, on = capi.default_opts(**RELAXED), capi.default_opts(chain_sites=1, **RELAXED)
    ids = np.arange(len(planted["queries"]), dtype=np.int32)
    batch = lambda t, p, o: t.merge(db, p, o)
    run = lambda t, p, o: t.merge(qb, p, ids, o)
    make, merge, finish_args = {"top": (lambda: capi.TopSet(ctx, qb, 3), batch, ()), "tophits": (lambda: capi.TopHits(ctx, qb, 3), batch, ()),
                                "profile": (lambda: capi.ProfSet(ctx, qb), batch, ()), "targets": (lambda: capi.TargetSet(ctx, db, 3), run, ()),
                                "coverage": (lambda: capi.CovSet(ctx, db), run, (1,))}[kind]
    try:
        # a table fed pages with 0 and then 1: refused and left unchanged (the page can still be merged with 0)
        with make() as t, make() as ref:
            merge(t, 0, off)
            with pytest.raises(capi.PrbError, match="chain_sites 0 .this call: 1"):
                merge(t, 1, on)
            for p in range(1, db.npages):
                merge(t, p, off)
            for p in range(db.npages):
                merge(ref, p, off)
            assert t.counts() == ref.counts()
            a, b = t.finish(*finish_args), ref.finish(*finish_args)
            a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        # a 0-table and a 1-table do not merge; an empty table takes either and carries the value over
        with make() as t0, make() as t1, make() as empty:
            merge(t0, 0, off)
            merge(t1, 1, on)
            with pytest.raises(capi.PrbError, match="chain_sites 0 and 1"):
                t0.absorb(t1)
            with pytest.raises(capi.PrbError, match="chain_sites 1 and 0"):
                t1.absorb(t0)
            empty.absorb(t1)
            with pytest.raises(capi.PrbError, match="chain_sites"):
                merge(empty, 2, off)
            merge(empty, 2, on)
    finally:
        qb.close()
        db.close()
