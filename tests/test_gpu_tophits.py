"""GPU tests of the top-N hit mode (prb_search_page_tophits, `ris -k N`): each query's N final hits of lowest interaction
energy, kept with their base pairs in a table on the device that every page of a batch is merged into.  The yardstick
is the hit path, prb_search_page over all pages (pinned to the reference by test_gpu_search.py / test_gpu_options.py),
ranked here in Python: a query's hits concatenated in page order, stable-sorted by e_tot, cut to N, their base-pair
lists laid end to end.  The table must match it byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refdump
from test_gpu_options import OPTION_SETS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
OPTS = [{}, OPTION_SETS[1], OPTION_SETS[5]]  # defaults; -f -2 -g -5; -m 2

K_TOP_TILE = 1024  # records a k_top_merge workgroup streams per step (table_kernels.hip, kTopTile)


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


class Ranking:
    """The contract restated.  pages = [(hits HIT_DTYPE, bp int32 [npairs, 2]) of page p, or None for a page left out]:
    every query's hits ordered by (e_tot as a double, page, place among the page's hits)."""

    def __init__(self, pages):
        self.pages = pages
        hits = [p[0] for p in pages if p is not None]
        self.page = np.concatenate([np.full(len(p[0]), k, np.int32) for k, p in enumerate(pages) if p is not None] or
                                   [np.zeros(0, np.int32)])
        self.place = np.concatenate([np.arange(len(h), dtype=np.int64) for h in hits] or [np.zeros(0, np.int64)])
        self.query = np.concatenate([h["query"] for h in hits] or [np.zeros(0, np.int32)])
        e = np.concatenate([h["e_tot"] for h in hits] or [np.zeros(0)]) + 0.0  # (-0.0 + 0.0 = +0.0: the two compare equal)
        self.order = np.lexsort((self.place, self.page, e, self.query))
        self.total = len(self.order)

    def cut(self, n):
        """-> (TOPHIT_DTYPE records by query, then rank; their base pairs, end to end)"""
        from priblast_amd import capi
        q = self.query[self.order]
        start = np.searchsorted(q, q, side="left")  # first entry of each entry's query
        rank = np.arange(len(q)) - start
        keep = self.order[rank < n]
        out = np.zeros(len(keep), capi.TOPHIT_DTYPE)
        lists, at = [], 0
        for i, (k, r) in enumerate(zip(keep, rank[rank < n])):
            hits, bp = self.pages[int(self.page[k])]
            h = hits[int(self.place[k])]
            for f in capi.HIT_DTYPE.names:
                out[i][f] = h[f]
            lists.append(bp[int(h["bp_offset"]):int(h["bp_offset"]) + int(h["bp_count"])])
            out[i]["bp_offset"], out[i]["page"], out[i]["rank"] = at, int(self.page[k]), int(r)
            at += int(h["bp_count"])
        pairs = np.concatenate(lists).astype(np.int32) if lists else np.zeros((0, 2), np.int32)
        return out, pairs.reshape(-1, 2)


def hit_pages(ctx, qb, db, opts, pages=None):
    """the hit path: [(hits, bp, counts) of page p] (copies)"""
    from priblast_amd import capi
    out = []
    for p in range(db.npages):
        if pages is not None and p not in pages:
            out.append(None)
            continue
        hits, bp, counts = capi.search_page(ctx, qb, db, p, opts)
        out.append((hits.copy(), bp.copy(), counts))
    return out


def open_batch(ctx, prefix, seqs, max_resident_pages=None):
    from priblast_amd import capi
    db = capi.Db(ctx, prefix, max_resident_pages)
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    return db, qb


def assert_bytes(got, want, what):
    (grec, gbp), (wrec, wbp) = got, want
    assert len(grec) == len(wrec), (what, len(grec), len(wrec))
    if grec.tobytes() != wrec.tobytes():
        for k in range(len(grec)):
            assert grec[k].tobytes() == wrec[k].tobytes(), (what, k, grec[k], wrec[k])
    assert gbp.shape == wbp.shape and gbp.tobytes() == wbp.tobytes(), (what, "base pairs")


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


def test_tophits_equal_ranked_hits(ctx, golden_dir):
    from priblast_amd import capi
    dropped = 0
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
        try:
            for kw in OPTS:
                for style in (0, 1):
                    opts = capi.default_opts(output_style=style, **kw)
                    pages = hit_pages(ctx, qb, db, opts)
                    ranking = Ranking([(h, bp) for h, bp, _ in pages])
                    most = int(np.bincount(ranking.query).max()) if ranking.total else 1
                    for n in (1, 2, 3, most, most + 5):
                        recs, bp, counts = capi.search_tophits(ctx, qb, db, n, opts, with_counts=True)
                        assert counts == tuple(int(sum(c[i] for _, _, c in pages)) for i in range(3))
                        want = ranking.cut(n)
                        assert_bytes((recs, bp), want, (tag, kw, style, n))
                        dropped += len(want[0]) < ranking.total
        finally:
            qb.close()
            db.close()
    assert dropped > 0


def test_tophits_select_over_many_tiles(ctx, tmp_path):
    """thousands of hits per query and page: each launch streams several steps, the candidate buffer is flushed in
    mid-stream, and between pages the pool of base pairs is rebuilt from survivors and newcomers mixed (middle N), from
    newcomers alone (N = 1 when a later page wins) and from survivors alone (the short query's few hits)"""
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    nseq, per_page = 3000, 1000
    prefix = str(tmp_path / "randdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(nseq)], [random_seq(rng, 500) for _ in range(nseq)], page_size=per_page)
    queries = [random_seq(rng, int(rng.integers(2000, 3001))) for _ in range(3)] + ["GGGAAACCCUUUAGCU" * 2]
    db, qb = open_batch(ctx, prefix, queries)
    try:
        assert db.npages == 3
        opts = capi.default_opts(output_style=1)
        ranking = Ranking([(h, bp) for h, bp, _ in hit_pages(ctx, qb, db, opts)])
        per = np.array([np.bincount(p[0]["query"], minlength=len(queries)) for p in ranking.pages])  # [page, query]
        print("hits per page and query:", per.tolist())
        assert per[:, :3].min() > 2 * K_TOP_TILE, per
        assert per[:, 3].sum() < 1024, per
        for n in (1, 63, 64, 65, 255, 256, 1000, 1024):
            want = ranking.cut(n)
            fwd = capi.search_tophits(ctx, qb, db, n, opts)
            assert_bytes(fwd, want, n)
            assert same_bytes(fwd, capi.search_tophits(ctx, qb, db, n, opts, pages=[2, 1, 0])), n
            assert same_bytes(fwd, capi.search_tophits(ctx, qb, db, n, opts, pages=[1, 2, 0])), n
    finally:
        qb.close()
        db.close()


def test_tophits_ties(ctx, tmp_path):
    """the same target twice in page 0 and once more in page 1: three hits of bit-identical e_tot; within a page the
    lower place wins, across pages the lower page, whatever the order of the merges"""
    from priblast_amd import capi
    site = "CCACCACACCCAACCACACC"
    comp = site[::-1].translate(str.maketrans("AC", "UG"))
    target = "C" * 30 + site + "C" * 30
    prefix = str(tmp_path / "tiedb")
    capi.db_build(ctx, prefix, ["copy_a", "copy_b", "copy_c", "decoy"], [target, target, target, "ACGU" * 25], page_size=2)
    db, qb = open_batch(ctx, prefix, ["UUUUUUUUUU" + comp + "UUUUUUUUUU"])
    try:
        assert db.npages == 2
        for style in (0, 1):
            opts = capi.default_opts(output_style=style)
            pages = [(h, bp) for h, bp, _ in hit_pages(ctx, qb, db, opts)]
            bits = [p[0]["e_tot"].view(np.uint64) for p in pages]
            best = np.float64(min(float(p[0]["e_tot"].min()) for p in pages)).view(np.uint64)
            tied = [np.flatnonzero(b == best) for b in bits]  # the hits of lowest e_tot: bit-identical
            assert len(tied[0]) == 2 and len(tied[1]) == 1, tied
            ranking = Ranking(pages)
            for order in ([0, 1], [1, 0]):
                for n in (1, 2, 3):
                    got = capi.search_tophits(ctx, qb, db, n, opts, pages=order)
                    assert_bytes(got, ranking.cut(n), (style, order, n))
                    assert [int(p) for p in got[0]["page"]] == [0, 0, 1][:n]
                    firsts = [pages[0][0][tied[0][0]], pages[0][0][tied[0][1]], pages[1][0][tied[1][0]]]
                    for k in range(n):
                        assert int(got[0][k]["db_sp"]) == int(firsts[k]["db_sp"]), (style, order, n, k)
    finally:
        qb.close()
        db.close()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "PRB_TRACE_NO_SLOTS=1", "resident=1"])
def test_tophits_invariance(ctx, golden_dir, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; every final hit re-extended for its base
    pairs; the 3-page database streamed through one resident page: the same bytes"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    prefix = os.path.join(golden_dir, "mixdb")
    opts = capi.default_opts(output_style=1)
    db, qb = open_batch(ctx, prefix, seqs)
    try:
        plain = {n: capi.search_tophits(ctx, qb, db, n, opts) for n in (1, 3)}
    finally:
        qb.close()
        db.close()
    assert sum(len(v[0]) for v in plain.values()) > 10 and all(len(v[1]) > len(v[0]) for v in plain.values())
    name, value = knob.split("=")
    if name != "resident":
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, prefix, seqs, int(value) if name == "resident" else None)
    try:
        for n, want in plain.items():
            assert same_bytes(capi.search_tophits(ctx, qb, db, n, opts), want), (knob, n)
    finally:
        qb.close()
        db.close()


def test_tophits_edges(ctx, golden_dir):
    from priblast_amd import capi
    prefix = os.path.join(golden_dir, "mixdb")
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    # a query without hits gives no records
    db, qb = open_batch(ctx, prefix, ["A" * 60])
    try:
        recs, bp, counts = capi.search_tophits(ctx, qb, db, 5, with_counts=True)
        assert len(recs) == 0 and len(bp) == 0 and counts[2] == 0
    finally:
        qb.close()
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    other = capi.QBatch(ctx, seqs[:2], db.repeat_flag)
    other.accessibility(db.W, db.delta)
    try:
        for n in (0, -1, 1025):
            with pytest.raises(capi.PrbError):
                capi.TopHits(ctx, qb, n)
        with capi.TopHits(ctx, qb, 2) as th:
            th.merge(db, 1)
            with pytest.raises(capi.PrbError, match="already merged"):
                th.merge(db, 1)
        # a call refused by the argument checks leaves the table as it was: the page can still be merged
        style1 = capi.default_opts(output_style=1)
        ranking = Ranking([(h, bp) for h, bp, _ in hit_pages(ctx, qb, db, style1)])
        with capi.TopHits(ctx, qb, 2) as th:
            with pytest.raises(capi.PrbError, match="unsupported option"):
                th.merge(db, 0, capi.default_opts(output_style=1, drop_out_w_gap=31))
            with pytest.raises(capi.PrbError):
                th.merge(db, db.npages)
            th.merge(db, 0, style1)
            with pytest.raises(capi.PrbError, match="output_style"):  # every merge with the same style
                th.merge(db, 1, capi.default_opts(output_style=0))
            for p in range(1, db.npages):
                th.merge(db, p, style1)
            got = th.finish()
            assert_bytes(got, ranking.cut(2), "after refused calls")
            # finished: the device table is gone, a second finish changes nothing, no page can be merged
            assert same_bytes(th.finish(), got)
            with pytest.raises(capi.PrbError, match="finished"):
                th.merge(db, 0, style1)
        with capi.TopHits(ctx, other, 2) as th:  # a table made for another batch
            with pytest.raises(capi.PrbError, match="another context or query batch"):
                capi._check(capi.lib().prb_search_page_tophits(ctx.h, qb.h, db.h, 0, ctypes.byref(capi.default_opts()), th.h))
        # pages left out are simply not in the table
        with capi.TopHits(ctx, qb, 2) as th:
            th.merge(db, 2, style1)
            th.merge(db, 0, style1)
            want = Ranking([ranking.pages[0], None, ranking.pages[2]]).cut(2)
            assert_bytes(th.finish(), want, "pages 0 and 2")
    finally:
        qb.close()
        other.close()
        db.close()


def run_ris(golden_dir, tmp_path, tag, name, extra=(), env_extra=None):
    from priblast_amd import capi
    out = str(tmp_path / name)
    env = dict(os.environ, PRB_BATCH="5", **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, f"{tag}_q.fa"), "-o", out, "-d",
                    os.path.join(golden_dir, f"{tag}db")] + list(extra), check=True, env=env, timeout=600)
    return out


def read(path):
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize("tag", ["mix", "quirk"])
def test_cli_tophits_lines(ctx, golden_dir, tmp_path, tag):
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    # the C ABI's hits ranked in Python, batch by batch as the command line cuts them (longest queries first, 5 a batch)
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
    db = capi.Db(ctx, os.path.join(golden_dir, f"{tag}db"))
    per_batch = []
    try:
        for b0 in range(0, len(order), 5):
            idx = order[b0:b0 + 5]
            qb = capi.QBatch(ctx, [seqs[i] for i in idx], db.repeat_flag)
            qb.accessibility(db.W, db.delta)
            try:
                per_batch.append((idx, Ranking([(h, bp) for h, bp, _ in hit_pages(ctx, qb, db, capi.default_opts())])))
            finally:
                qb.close()
        for style in ("0", "1"):
            full = read(run_ris(golden_dir, tmp_path, tag, f"full{style}.txt", ["-s", style])).splitlines()
            plain = {l.split(",", 1)[1] for l in full[3:]}
            for n in (1, 3):
                text = read(run_ris(golden_dir, tmp_path, tag, f"k{n}s{style}.txt", ["-k", str(n), "-s", style]))
                lines = text.splitlines()
                assert lines[:3] == full[:3]
                body = lines[3:]
                assert len(body) > 0 and [int(l.split(",", 1)[0]) for l in body] == list(range(len(body)))
                assert all(l.split(",", 1)[1] in plain for l in body)
                want = []
                for idx, ranking in per_batch:
                    for r in ranking.cut(n)[0]:
                        want.append((names[idx[int(r["query"])]], db.seq_name(int(r["page"]), int(r["db_id"])), "%g" % r["e_tot"]))
                assert [(l.split(",")[1], l.split(",")[3], l.split(",")[7]) for l in body] == want
            # (text = -k 3 with this style; two workers with the end pairs, the binary records with every pair)
            if style == "0":
                two = run_ris(golden_dir, tmp_path, tag, "two.txt", ["-k", "3", "-s", style], {"PRB_DEVICES": "0,0"})
                assert read(two) == text
            else:
                binary = run_ris(golden_dir, tmp_path, tag, "k3.prb", ["-k", "3", "-s", style, "-b"])
                back = str(tmp_path / "back.txt")
                subprocess.run([capi.BIN_PATH, "txt", "-i", binary, "-o", back], check=True, timeout=600)
                assert read(back) == text
    finally:
        db.close()
