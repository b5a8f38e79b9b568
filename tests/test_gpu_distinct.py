"""GPU tests of opts.distinct_sites (`ris -u`) through the search.  The yardstick is the plain hit path - prb_search_page
with distinct_sites = 0, pinned to the reference by test_gpu_search.py / test_gpu_options.py - filtered in Python by the
rule of include/priblast_hip.h (distinct_ref.filter_page); the other modes are compared with the existing Python
restatements of their contracts over those filtered hits."""
import os

import numpy as np
import pytest

import refdump
from distinct_ref import filter_page, keep_mask, planted_sequences, runs_of
from test_gpu_options import OPTION_SETS
from test_gpu_profile import profile
from test_gpu_summary import assert_same, reduce_hits
from test_gpu_top import rank
from test_gpu_tophits import Ranking, assert_bytes, open_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
OPTS = [{}, OPTION_SETS[1], OPTION_SETS[5]]  # defaults; -f -2 -g -5; -m 2 (what test_gpu_tophits.py uses)
RELAXED = dict(interaction_threshold=-3.0, final_threshold=-6.5)  # -f -3 -g -6.5 (distinct_ref.planted_sequences)


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def search(ctx, qb, db, opts):
    """[(hits, bp, counts)] per page, copies"""
    from priblast_amd import capi
    out = []
    for p in range(db.npages):
        hits, bp, counts = capi.search_page(ctx, qb, db, p, opts)
        out.append((np.array(hits), np.array(bp).reshape(-1, 2), counts))
    return out


def assert_pages(got, want, what):
    assert len(got) == len(want)
    for p, ((gh, gbp, gc), (wh, wbp, wc)) in enumerate(zip(got, want)):
        assert gc[2] == wc[2] and tuple(gc) == tuple(wc), (what, p, gc, wc)  # counts[2]: before the selection
        assert_bytes((gh, gbp), (wh, wbp), (what, p))


def filtered(plain):
    """the yardstick: [(hits, bp, counts of the plain search)] per page"""
    return [filter_page(h, bp)[:2] + (c,) for h, bp, c in plain]


def test_goldens(ctx, golden_dir):
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
                    got = search(ctx, qb, db, capi.default_opts(output_style=style, distinct_sites=1, **kw))
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
    prefix = str(tmp_path_factory.mktemp("planted") / "pdb")
    capi.db_build(ctx, prefix, tnames, targets, page_size=7)
    db, qb = open_batch(ctx, prefix, queries)
    try:
        assert db.npages == 3
        plain = {style: search(ctx, qb, db, capi.default_opts(output_style=style, **RELAXED)) for style in (0, 1)}
    finally:
        qb.close()
        db.close()
    return dict(prefix=prefix, qnames=qnames, queries=queries, plain=plain, want={s: filtered(p) for s, p in plain.items()})


def test_planted_case_has_dense_runs(planted):
    """what the other tests lean on, on the PLAIN output: without it a library that ignored the option could pass"""
    lengths, total, kept, witness = [], 0, 0, 0
    for hits, _, _ in planted["plain"][0]:
        keep = keep_mask(hits)
        total += len(hits)
        kept += int(keep.sum())
        q1, d1 = hits["q_sp"] + hits["q_len"] - 1, hits["db_sp"] + hits["db_len"] - 1
        for a, b in runs_of(hits):
            lengths.append(b - a)
            for i in np.flatnonzero(~keep[a:b]) + a:
                k = np.flatnonzero(keep[a:b]) + a
                witness += int(((hits["q_sp"][k] <= q1[i]) & (hits["q_sp"][i] <= q1[k]) & (hits["db_sp"][k] <= d1[i]) &
                                (hits["db_sp"][i] <= d1[k])).any())
    lengths = np.array(lengths)
    print("planted case: hits", total, "kept", kept, "runs", len(lengths), "longest", int(lengths.max()), "singletons",
          int((lengths == 1).sum()), "runs of 2..63", int(((lengths >= 2) & (lengths <= 63)).sum()), "runs above 64",
          int((lengths > 64).sum()))
    assert (lengths > 64).any()
    assert ((lengths >= 2) & (lengths <= 63)).any()
    assert (lengths == 1).any()
    assert total - kept >= total / 4
    assert witness > 0  # a kept hit intersects a dropped hit of its pair (every dropped hit has one: the rule)
    assert witness == total - kept


KNOBS = ["plain", "PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=37", "resident=1", "PRB_DISTINCT_LDS_HITS=1", "PRB_DISTINCT_LDS_HITS=40"]


@pytest.mark.parametrize("knob", KNOBS)
def test_planted_hits_and_invariance(ctx, planted, monkeypatch, knob):
    """the kept hits, byte for byte, for both output styles - whatever cuts the batch, chunks the gapped stage, streams
    the pages or moves the selection's state to HBM"""
    from priblast_amd import capi
    name, _, value = knob.partition("=")
    if name.startswith("PRB_"):
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"], int(value) if name == "resident" else None)
    try:
        for style in (0, 1):
            ctx.reset_timers()
            got = search(ctx, qb, db, capi.default_opts(output_style=style, distinct_sites=1, **RELAXED))
            assert_pages(got, planted["want"][style], (knob, style))
            assert sum(len(g[0]) for g in got) < sum(g[2][2] for g in got)  # size below counts[2]: hits were dropped
            assert ctx.stage_ms("distinct")[1] > 0
        if name == "plain":  # the timer stays silent without the option
            ctx.reset_timers()
            search(ctx, qb, db, capi.default_opts(**RELAXED))
            assert ctx.stage_ms("distinct") == (0.0, 0)
            # last_stage 1 and 2 ignore the field
            for stage in (1, 2):
                a = capi.search_page(ctx, qb, db, 0, capi.default_opts(distinct_sites=1, **RELAXED), stage)
                b = capi.search_page(ctx, qb, db, 0, capi.default_opts(**RELAXED), stage)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
            assert ctx.stage_ms("distinct") == (0.0, 0)
    finally:
        qb.close()
        db.close()


def pair_records(hits, bp):
    """reduce_hits' dictionaries as PAIR_DTYPE records"""
    from priblast_amd import capi
    red = reduce_hits(hits, bp)
    out = np.zeros(len(red), capi.PAIR_DTYPE)
    for i, r in enumerate(red):
        for f in ("query", "db_id", "hits", "e_min", "e_sum", "e_acc", "e_hyb", "bp_first", "bp_last"):
            out[i][f] = r[f]
    return out


def test_planted_modes(ctx, planted):
    """-t, -t -n, -k and -q with the option on = their restatements over the filtered hits"""
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    want0, want1 = planted["want"][0], planted["want"][1]
    counts = tuple(int(sum(w[2][i] for w in want0)) for i in range(3))
    try:
        on0 = capi.default_opts(output_style=0, distinct_sites=1, **RELAXED)
        on1 = capi.default_opts(output_style=1, distinct_sites=1, **RELAXED)
        summed = 0
        for p in range(db.npages):
            pairs, c = capi.search_page_summary(ctx, qb, db, p, on0, with_counts=True)
            assert_same(pairs, reduce_hits(want0[p][0], want0[p][1]), ("summary", p))
            assert tuple(c) == tuple(want0[p][2])
            assert int(pairs["hits"].sum()) == len(want0[p][0]) <= c[2]
            summed += int(pairs["hits"].sum())
        assert summed < counts[2]  # hits were dropped (not on every page: one holds only the random targets)
        for n in (1, 3):
            recs, c = capi.search_top(ctx, qb, db, n, on0, with_counts=True)
            want = rank([pair_records(h, bp) for h, bp, _ in want0], n)
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
    finally:
        qb.close()
        db.close()


def test_refusals(ctx, planted):
    from priblast_amd import capi
    db, qb = open_batch(ctx, planted["prefix"], planted["queries"])
    off, on = capi.default_opts(**RELAXED), capi.default_opts(distinct_sites=1, **RELAXED)
    try:
        for bad in (2, -1):
            with pytest.raises(capi.PrbError, match="distinct_sites"):
                capi.search_page(ctx, qb, db, 0, capi.default_opts(distinct_sites=bad))
            with pytest.raises(capi.PrbError, match="distinct_sites"):
                capi.search_page_summary(ctx, qb, db, 0, capi.default_opts(distinct_sites=bad))
        tables = [lambda: capi.TopSet(ctx, qb, 3), lambda: capi.TopHits(ctx, qb, 3), lambda: capi.ProfSet(ctx, qb)]
        for make in tables:
            # a table fed pages with 0 and then 1: refused and left unchanged (the page can still be merged with 0)
            with make() as t, make() as ref:
                t.merge(db, 0, off)
                with pytest.raises(capi.PrbError, match="distinct_sites"):
                    t.merge(db, 1, on)
                for p in range(1, db.npages):
                    t.merge(db, p, off)
                for p in range(db.npages):
                    ref.merge(db, p, off)
                assert t.counts() == ref.counts()
                a, b = t.finish(), ref.finish()
                a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            # a 0-table and a 1-table do not merge; an empty table takes either
            with make() as t0, make() as t1, make() as empty:
                t0.merge(db, 0, off)
                t1.merge(db, 1, on)
                with pytest.raises(capi.PrbError, match="distinct_sites"):
                    t0.absorb(t1)
                with pytest.raises(capi.PrbError, match="distinct_sites"):
                    t1.absorb(t0)
                empty.absorb(t1)
                with pytest.raises(capi.PrbError, match="distinct_sites"):
                    empty.merge(db, 2, off)
                empty.merge(db, 2, on)
    finally:
        qb.close()
        db.close()
