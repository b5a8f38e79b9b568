"""GPU tests of opts.allowed_pairs (prb_pairmask, `ris -L`) through the C ABI.  The yardstick of a masked search is the
UNMASKED search of the same build - pinned to the reference by test_gpu_search.py / test_gpu_options.py - filtered to the
allowed pairs in numpy.  Hit records are compared field for field; base pairs in order, except for a hit that is the first
of its query's list in either run: its pairs keep the order they were found in, and the first hit of the
restricted list is another one than the first hit of the full list, so those are compared as sorted lists."""
import os

import numpy as np
import pytest

import refdump
from test_gpu_edge import DEGENERATE
from test_gpu_summary import assert_same, reduce_hits
from test_gpu_tophits import open_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIELDS = ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start", "e_acc", "e_hyb", "e_tot", "query", "bp_count")


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def search(ctx, qb, db, opts, last_stage=3):
    """[(hits, bp, counts)] per page, copies"""
    from priblast_amd import capi
    out = []
    for p in range(db.npages):
        hits, bp, counts = capi.search_page(ctx, qb, db, p, opts, last_stage)
        out.append((np.array(hits), np.array(bp).reshape(-1, 2), tuple(counts)))
    return out


def tbase_of(db):
    t = [0]
    for p in range(db.npages):
        t.append(t[-1] + db.page_info(p)[0])
    return t


def make_mask(ctx, qb, db, allowed):
    """allowed: bool [nq, ntargets] -> PairMask"""
    from priblast_amd import capi
    tb = np.array(tbase_of(db))
    m = capi.PairMask(ctx, qb, db)
    q, t = np.nonzero(allowed)
    page = np.searchsorted(tb, t, side="right") - 1
    if len(q):
        m.allow(q, page, t - tb[page])
    assert m.count == int(allowed.sum())
    return m


def first_flags(hits):
    q = hits["query"]
    return np.r_[True, q[1:] != q[:-1]] if len(q) else np.zeros(0, bool)


def assert_subset(got, plain, allowed, tbase, what):
    """got = the masked pages, plain = the unmasked ones"""
    assert len(got) == len(plain)
    for p, ((gh, gbp, _), (wh, wbp, _)) in enumerate(zip(got, plain)):
        keep = allowed[wh["query"], tbase[p] + wh["db_id"]] if len(wh) else np.zeros(0, bool)
        wfirst = first_flags(wh)[keep]
        wh = wh[keep]
        assert len(gh) == len(wh), (what, p, len(gh), len(wh))
        for f in FIELDS:
            assert gh[f].tobytes() == wh[f].tobytes(), (what, p, f)
        gfirst = first_flags(gh)
        for k in range(len(gh)):
            a = gbp[gh["bp_offset"][k]:gh["bp_offset"][k] + gh["bp_count"][k]]
            b = wbp[wh["bp_offset"][k]:wh["bp_offset"][k] + wh["bp_count"][k]]
            if gfirst[k] or wfirst[k]:
                a, b = np.array(sorted(map(tuple, a.tolist()))), np.array(sorted(map(tuple, b.tolist())))
            assert np.array_equal(a, b), (what, p, k)


# ------------------------------------------------------------------------- 1. the full mask is the identity
@pytest.mark.parametrize("tag", ["c1", "mix", "quirk"])
def test_full_mask_is_the_identity(ctx, golden_dir, tag):
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
    try:
        full = np.ones((len(seqs), tbase_of(db)[-1]), bool)
        with make_mask(ctx, qb, db, full) as m:
            for style in (0, 1):
                plain = search(ctx, qb, db, capi.default_opts(output_style=style))
                got = search(ctx, qb, db, capi.default_opts(output_style=style, allowed_pairs=m.h))
                for p, ((gh, gbp, gc), (wh, wbp, wc)) in enumerate(zip(got, plain)):
                    assert gc == wc, (tag, style, p, gc, wc)
                    assert gh.tobytes() == wh.tobytes() and gbp.tobytes() == wbp.tobytes(), (tag, style, p)
                assert sum(len(h) for h, _, _ in plain) > 0
    finally:
        qb.close()
        db.close()


# ------------------------------------------------------------------------- 2. exact subsets, both forms
@pytest.fixture(scope="module")
def wide(ctx, tmp_path_factory):
    """mix's 24 targets three times over under new names - 72 targets, so that the page-by-page numbering reaches 31, 32,
    63 and 64 - in pages whose first targets do not start a mask word; the unmasked hits of both output styles and the
    unmasked seeds, computed once with the default knobs and never changed"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    _, queries = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    tn = [f"{n}_copy{k}" for k in range(3) for n in names]
    ts = [s for k in range(3) for s in seqs]
    prefix = str(tmp_path_factory.mktemp("wide") / "wdb")
    capi.db_build(ctx, prefix, tn, ts, page_size=20)  # pages of 20 sequences: targets 0, 20, 40, 60
    db, qb = open_batch(ctx, prefix, queries)
    try:
        tb = tbase_of(db)
        assert db.npages >= 3 and tb[-1] == 72 and any(t % 32 for t in tb[1:-1]), tb
        plain = {style: search(ctx, qb, db, capi.default_opts(output_style=style)) for style in (0, 1)}
        seeds = search(ctx, qb, db, capi.default_opts(), last_stage=1)
    finally:
        qb.close()
        db.close()
    return dict(prefix=prefix, queries=queries, tbase=tb, plain=plain, seeds=seeds)


def masks_of(nq, nt, plain, tbase):
    rng = np.random.default_rng(7)
    hit = np.zeros((nq, nt), bool)  # the pairs with final hits
    for p, (h, _, _) in enumerate(plain):
        hit[h["query"], tbase[p] + h["db_id"]] = True
    out = {}
    m = np.zeros((nq, nt), bool)
    m[:, np.flatnonzero(hit.any(0))[0]] = True
    out["one_target"] = m
    m = np.zeros((nq, nt), bool)
    m[:, ::2] = True
    out["every_other_target"] = m
    m = np.zeros((nq, nt), bool)
    for q in range(nq):
        t = np.flatnonzero(hit[q])
        m[q, t[len(t) // 2] if len(t) else q] = True
    out["one_pair_per_query"] = m
    out["a_set_per_query"] = rng.random((nq, nt)) < 0.3
    m = np.zeros((nq, nt), bool)
    m[:, [31, 32, 63, 64]] = True
    out["word_edges"] = m
    m = np.zeros((nq, nt), bool)
    m[::2, 31] = m[1::2, 32] = m[::2, 64] = m[1::2, 63] = True
    out["word_edges_per_query"] = m
    return out


MASKS = ["one_target", "every_other_target", "one_pair_per_query", "a_set_per_query", "word_edges", "word_edges_per_query"]
KNOBS = ["plain", "PRB_SEED_FUSED=0", "PRB_SEARCH_PAIRS=1", "PRB_SEARCH_PAIRS=1 PRB_NO_FRONT_AHEAD=1", "PRB_SEED_ROW_SHIFT=-1"]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", MASKS)
def test_masked_search_is_the_filtered_search(ctx, wide, monkeypatch, name, knob):
    from priblast_amd import capi
    for kv in knob.split():
        if "=" in kv:
            monkeypatch.setenv(*kv.split("="))
    nq, nt = len(wide["queries"]), wide["tbase"][-1]
    allowed = masks_of(nq, nt, wide["plain"][0], wide["tbase"])[name]
    db, qb = open_batch(ctx, wide["prefix"], wide["queries"])
    try:
        with make_mask(ctx, qb, db, allowed) as m:
            for style in (0, 1):
                got = search(ctx, qb, db, capi.default_opts(output_style=style, allowed_pairs=m.h))
                assert_subset(got, wide["plain"][style], allowed, wide["tbase"], (name, knob, style))
            kept = sum(len(h) for h, _, _ in got)
            print(name, knob, "hits", kept, "of", sum(len(h) for h, _, _ in wide["plain"][1]))
            assert kept > 0
    finally:
        qb.close()
        db.close()


def test_a_chunk_emptied_and_a_chunk_untouched(ctx, wide, monkeypatch, capfd):
    """small chunks of candidates; a mask that allows one query everything and the others nothing empties every chunk of
    the other queries and leaves that query's untouched"""
    from priblast_amd import capi
    monkeypatch.setenv("PRB_SEARCH_CHUNK_PAIRS", "400")  # (a page has a few thousand pairs per query)
    monkeypatch.setenv("PRB_DEBUG_ROWS", "1")
    nq, nt = len(wide["queries"]), wide["tbase"][-1]
    allowed = np.zeros((nq, nt), bool)
    allowed[2] = True
    db, qb = open_batch(ctx, wide["prefix"], wide["queries"])
    try:
        capfd.readouterr()
        with make_mask(ctx, qb, db, allowed) as m:
            got = search(ctx, qb, db, capi.default_opts(output_style=1, allowed_pairs=m.h))
        lines = [l.split() for l in capfd.readouterr().err.splitlines() if l.startswith("[allow]")]
        assert_subset(got, wide["plain"][1], allowed, wide["tbase"], "chunks")
    finally:
        qb.close()
        db.close()
    pairs = np.array([int(l[4]) for l in lines])
    kept = np.array([int(l[6]) for l in lines])
    print("chunks", len(lines), "emptied", int((kept == 0).sum()), "untouched", int((kept == pairs).sum()))
    assert len(lines) > 3
    assert (kept == 0).any() and (kept == pairs).any()
    assert sum(len(h) for h, _, _ in got) > 0


# ------------------------------------------------------------------------- 3. the filter sits at the seeds
@pytest.mark.parametrize("name", ["every_other_target", "a_set_per_query", "word_edges_per_query"])
def test_filter_sits_at_the_seeds(ctx, wide, name):
    from priblast_amd import capi
    nq, nt = len(wide["queries"]), wide["tbase"][-1]
    allowed = masks_of(nq, nt, wide["plain"][0], wide["tbase"])[name]
    db, qb = open_batch(ctx, wide["prefix"], wide["queries"])
    try:
        with make_mask(ctx, qb, db, allowed) as m:
            o = capi.default_opts(allowed_pairs=m.h)
            seeds = search(ctx, qb, db, o, last_stage=1)
            final = search(ctx, qb, db, o)
    finally:
        qb.close()
        db.close()
    total = 0
    for p, ((gh, _, gc), (wh, _, _), (_, _, fc)) in enumerate(zip(seeds, wide["seeds"], final)):
        want = wh[allowed[wh["query"], wide["tbase"][p] + wh["db_id"]]]
        assert gc[0] == len(want) == fc[0], (name, p, gc, len(want), fc)
        assert gh.tobytes() == want.tobytes(), (name, p)
        total += len(want)
    assert 0 < total < sum(len(h) for h, _, _ in wide["seeds"])


# ------------------------------------------------------------------------- 4. empty and degenerate
def test_empty_and_degenerate(ctx, wide, golden_dir):
    """a mask whose bits are set only for pairs without a single seed - every target for a query of N's, which has no
    seed at all, and whatever pairs of the other queries the unmasked seed dump shows none for: empty in every mode"""
    from priblast_amd import capi
    seqs = wide["queries"] + ["N" * 40]
    nq, nt = len(seqs), wide["tbase"][-1]
    ids = np.arange(nq, dtype=np.int32)
    db, qb = open_batch(ctx, wide["prefix"], seqs)
    try:
        allowed = np.ones((nq, nt), bool)
        for p, (h, _, _) in enumerate(search(ctx, qb, db, capi.default_opts(), last_stage=1)):
            assert not (h["query"] == nq - 1).any()
            allowed[h["query"], wide["tbase"][p] + h["db_id"]] = False
        print("seedless pairs allowed:", int(allowed.sum()), "of them the N query's:", nt)
        assert allowed[nq - 1].all() and not allowed[:nq - 1].all()
        with make_mask(ctx, qb, db, allowed) as m:
            o = capi.default_opts(allowed_pairs=m.h)
            for stage in (1, 2, 3):
                for h, bp, c in search(ctx, qb, db, o, last_stage=stage):
                    assert len(h) == 0 and len(bp) == 0 and c == (0, 0, 0)
            for p in range(db.npages):
                assert len(capi.search_page_summary(ctx, qb, db, p, o)) == 0
            assert len(capi.search_top(ctx, qb, db, 3, o)) == 0
            recs, bp = capi.search_tophits(ctx, qb, db, 5, o)
            assert len(recs) == 0 and len(bp) == 0
            assert len(capi.search_profile(ctx, qb, db, o)) == 0
            assert len(capi.search_targets(ctx, db, 2, [(qb, ids)], o)) == 0
            assert len(capi.search_coverage(ctx, db, 1, [(qb, ids)], o)) == 0
            for flag in ("distinct_sites", "chain_sites"):
                assert sum(len(h) for h, _, _ in search(ctx, qb, db, capi.default_opts(allowed_pairs=m.h, **{flag: 1}))) == 0
    finally:
        qb.close()
    try:
        qb = capi.QBatch(ctx, wide["queries"][3:4], db.repeat_flag)  # a one-query batch
        qb.accessibility(db.W, db.delta)
        allowed = np.zeros((1, nt), bool)
        allowed[0, 1::3] = True
        ref = search(ctx, qb, db, capi.default_opts(output_style=1))
        with make_mask(ctx, qb, db, allowed) as m:
            got = search(ctx, qb, db, capi.default_opts(output_style=1, allowed_pairs=m.h))
        assert_subset(got, ref, allowed, wide["tbase"], "one query")
        qb.close()
        seqs = DEGENERATE + wide["queries"][:2]
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        allowed = np.zeros((len(seqs), nt), bool)
        allowed[:, ::3] = True
        ref = search(ctx, qb, db, capi.default_opts(output_style=1))
        with make_mask(ctx, qb, db, allowed) as m:
            got = search(ctx, qb, db, capi.default_opts(output_style=1, allowed_pairs=m.h))
        assert_subset(got, ref, allowed, wide["tbase"], "degenerate")
        assert sum(len(h) for h, _, _ in got) > 0
    finally:
        qb.close()
        db.close()


# ------------------------------------------------------------------------- 5. the quirk
def test_first_hit_quirk_is_that_of_the_restricted_list(ctx, tmp_path):
    """quirk's sequences as a one-page database (prb_db_build); `ris -s 1 -L` with a mask that leaves out one target =
    the plain `ris -s 1` against a one-page database built from the other sequences in the same order, as sorted lines
    without Id - base pairs as text, in the order printed: the restricted list's first hit is the subset database's.
    Left out in turn: kd0, the target of the full run's hit 0 (the only hit of its query), and kdecoy0, behind which
    other hits become the first of their lists.
    Checked beforehand on the CPU with the oracle (reference-built one-page databases, `-s 1`): its run on either subset
    database equals its full run filtered by target name once every line's base pairs are sorted - seeds do not depend on
    the database's composition - and without kdecoy0 the lines of kq1-kd1 and kq2-kd2 list their pairs in another order
    than in the full run: the quirk moving to another hit, which the equality below pins."""
    import subprocess
    import oraclelib
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "quirk_db.fa"))
    qfa = os.path.join(GOLDEN, "quirk_q.fa")
    qnames, _ = refdump.read_fasta(qfa)
    full = str(tmp_path / "full")
    capi.db_build(ctx, full, names, seqs)
    lines = 0
    for drop in ("kd0", "kdecoy0"):
        assert drop in names
        keep = [k for k, n in enumerate(names) if n != drop]
        sub = str(tmp_path / f"without_{drop}")
        capi.db_build(ctx, sub, [names[k] for k in keep], [seqs[k] for k in keep])
        lst = tmp_path / f"{drop}.tsv"
        lst.write_text("".join(f"*\t{names[k]}\n" for k in keep))
        subprocess.run([capi.BIN_PATH, "ris", "-i", qfa, "-s", "1", "-d", full, "-L", str(lst), "-o", str(tmp_path / "masked.out")], check=True)
        subprocess.run([capi.BIN_PATH, "ris", "-i", qfa, "-s", "1", "-d", sub, "-o", str(tmp_path / "subset.out")], check=True)
        a, b = oraclelib.sorted_body(str(tmp_path / "masked.out")), oraclelib.sorted_body(str(tmp_path / "subset.out"))
        assert a == b and len(a) > 0, drop
        assert not any(l.split(",")[2] == drop for l in a)
        lines += len(a)
    print("lines compared:", lines)


# ------------------------------------------------------------------------- 6. modes
def test_modes_take_the_restricted_list(ctx, wide):
    """-t, -t -n 3, -q, -k 5, -r 2, -c 1, -u and -j under one mixed mask = the existing Python restatements of each mode
    over the restricted hit list - the masked search's own list, which is first shown to be the unmasked list filtered"""
    import chain_ref
    import distinct_ref
    import test_gpu_coverage as cov
    import test_gpu_targets as tgt
    from test_gpu_distinct import pair_records
    from test_gpu_profile import profile
    from test_gpu_top import rank
    from test_gpu_tophits import Ranking, assert_bytes
    from priblast_amd import capi
    nq, nt = len(wide["queries"]), wide["tbase"][-1]
    allowed = masks_of(nq, nt, wide["plain"][0], wide["tbase"])["a_set_per_query"]
    ids = np.arange(nq, dtype=np.int32)
    db, qb = open_batch(ctx, wide["prefix"], wide["queries"])
    try:
        with make_mask(ctx, qb, db, allowed) as m:
            on0, on1 = capi.default_opts(output_style=0, allowed_pairs=m.h), capi.default_opts(output_style=1, allowed_pairs=m.h)
            want0, want1 = search(ctx, qb, db, on0), search(ctx, qb, db, on1)
            assert_subset(want0, wide["plain"][0], allowed, wide["tbase"], "style 0")
            assert_subset(want1, wide["plain"][1], allowed, wide["tbase"], "style 1")
            counts = tuple(int(sum(w[2][i] for w in want0)) for i in range(3))
            assert sum(len(h) for h, _, _ in want0) > 20
            pair_pages = [pair_records(h, bp) for h, bp, _ in want0]
            for p in range(db.npages):  # -t
                pairs, c = capi.search_page_summary(ctx, qb, db, p, on0, with_counts=True)
                assert_same(pairs, reduce_hits(want0[p][0], want0[p][1]), ("summary", p))
                assert tuple(c) == want0[p][2]
            recs, c = capi.search_top(ctx, qb, db, 3, on0, with_counts=True)  # -t -n 3
            assert recs.tobytes() == rank(pair_pages, 3).tobytes() and c == counts
            for opts, want in ((on0, want0), (on1, want1)):  # -k 5
                recs, bp, c = capi.search_tophits(ctx, qb, db, 5, opts, with_counts=True)
                assert_bytes((recs, bp), Ranking([(h, b) for h, b, _ in want]).cut(5), ("tophits", opts.output_style))
                assert c == counts
            rows, c = capi.search_profile(ctx, qb, db, on0, with_counts=True)  # -q
            pages = []
            for p, (h, bp, _) in enumerate(want0):
                off = h["bp_offset"].astype(np.int64)
                pages.append((p, h, bp[off], bp[off + 1]))
            assert rows.tobytes() == profile(pages, [len(q) for q in wide["queries"]]).tobytes() and c == counts
            got, c = capi.search_targets(ctx, db, 2, [(qb, ids)], on0, with_counts=True)  # -r 2
            tgt.assert_bytes(got, tgt.rank([(ids, p, recs) for p, recs in enumerate(pair_pages)], 2), "targets")
            assert c == counts
            info = cov.seq_info(db)  # -c 1
            tab = cov.table([(ids, p, h, bp) for p, (h, bp, _) in enumerate(want0)], info)
            got, c = capi.search_coverage(ctx, db, 1, [(qb, ids)], on0, with_counts=True)
            tgt.assert_bytes(got, cov.regions(tab, info, 1), "coverage")
            assert c == counts
            dropped = 0
            for flag, ref in (("distinct_sites", distinct_ref), ("chain_sites", chain_ref)):  # -u, -j
                thin = search(ctx, qb, db, capi.default_opts(output_style=1, allowed_pairs=m.h, **{flag: 1}))
                for p, ((gh, gbp, gc), (wh, wbp, wc)) in enumerate(zip(thin, want1)):
                    assert gc == wc, (flag, p)
                    assert_bytes((gh, gbp), ref.filter_page(wh, wbp)[:2], (flag, p))
                    dropped += len(wh) - len(gh)
            assert dropped > 0
    finally:
        qb.close()
        db.close()


# ------------------------------------------------------------------------- 7. refusals
def test_refusals(ctx, wide, golden_dir):
    from priblast_amd import capi
    db, qb = open_batch(ctx, wide["prefix"], wide["queries"])
    db2, qb2 = open_batch(ctx, os.path.join(golden_dir, "mixdb"), wide["queries"][:3])
    try:
        nq, nt = len(wide["queries"]), wide["tbase"][-1]
        m = capi.PairMask(ctx, qb, db)
        for q, p, d in ((nq, 0, 0), (-2, 0, 0), (0, db.npages, 0), (0, -1, 0), (0, 0, db.page_info(0)[0]), (0, 0, -1)):
            with pytest.raises(capi.PrbError, match="entry 1 is out of range"):
                m.allow([0, q], [0, p], [0, d])
            assert m.count == 0  # nothing of a refused call is applied
        m.allow([-1, 1, 1], [0, 1, 1], [2, 0, 0])
        assert m.count == nq + 1
        o = capi.default_opts(allowed_pairs=m.h)
        for other_qb, other_db in ((qb2, db), (qb, db2)):
            with pytest.raises(capi.PrbError, match="another query batch or another database"):
                capi.search_page(ctx, other_qb, other_db, 0, o)
        m.allow([0], [0], [0])  # not used yet: still open
        capi.search_page(ctx, qb, db, 0, o)
        with pytest.raises(capi.PrbError, match="before its first use only"):
            m.allow([0], [0], [1])
        m.close()
    finally:
        qb.close()
        qb2.close()
        db.close()
        db2.close()
