"""GPU tests of the top-N mode (prb_search_page_top, `ris -t -n N`): each query's N pairs of lowest minimum interaction
energy, kept in a table on the device that every page of a batch is merged into.  The yardstick is the per-pair
summary search over all pages (pinned to the hit path by test_gpu_summary.py), ranked here in Python: a query's
records concatenated in page order, stable-sorted by e_min, cut to N.  The table must match it byte for byte."""
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


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def rank(pages, n):
    """The contract restated: pages = [PAIR_DTYPE records of page p] -> TOP_DTYPE records, query by query, by rank."""
    from priblast_amd import capi
    per_q = {}
    for p, recs in enumerate(pages):
        for r in recs:
            per_q.setdefault(int(r["query"]), []).append((float(r["e_min"]), p, r))
    chosen = []
    for q in sorted(per_q):
        ranked = sorted(per_q[q], key=lambda t: t[0])  # stable: page, then position in the page (-0.0 == +0.0)
        chosen += [(p, k, r) for k, (_, p, r) in enumerate(ranked[:n])]
    out = np.zeros(len(chosen), capi.TOP_DTYPE)
    for i, (p, k, r) in enumerate(chosen):
        for f in capi.PAIR_DTYPE.names:
            out[i][f] = r[f]
        out[i]["page"], out[i]["rank"] = p, k
    return out


def summaries(ctx, qb, db, opts):
    from priblast_amd import capi
    return [capi.search_page_summary(ctx, qb, db, p, opts, with_counts=True) for p in range(db.npages)]


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


K_TOP_TILE = 1024  # records a k_top_merge workgroup streams per step (table_kernels.hip, kTopTile)


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


def random_db(ctx, tmp_path, nseq=12000, length=500, page_size=4000, seed=7):
    """three pages of 4,000 random 500-nt targets and six random 2-3 kb queries: nearly every (query, target) pair has
    a final hit, so a query's run against one page is several thousand records - several steps of the merge kernel,
    with flushes of the candidate buffer in between"""
    from priblast_amd import capi
    rng = np.random.default_rng(seed)
    seqs = [random_seq(rng, length) for _ in range(nseq)]
    prefix = str(tmp_path / "randdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(nseq)], seqs, page_size=page_size)
    queries = [random_seq(rng, int(rng.integers(2000, 3001))) for _ in range(6)]
    return prefix, queries


def test_top_equals_ranked_summaries(ctx, golden_dir):
    from priblast_amd import capi
    selected = 0
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
        try:
            for kw in OPTS:
                opts = capi.default_opts(**kw)
                pages = summaries(ctx, qb, db, opts)
                recs = [r for r, _ in pages]
                allrec = np.concatenate(recs)
                most = int(np.bincount(allrec["query"]).max()) if len(allrec) else 1
                for n in (1, 2, 3, most, most + 5):
                    got, counts = capi.search_top(ctx, qb, db, n, opts, with_counts=True)
                    assert counts == tuple(int(sum(c[i] for _, c in pages)) for i in range(3))
                    want = rank(recs, n)
                    assert_bytes(got, want, (tag, kw, n))
                    selected += len(want) < sum(len(r) for r in recs)
        finally:
            qb.close()
            db.close()
    assert selected > 0


def test_top_selects_over_many_tiles(ctx, tmp_path):
    """thousands of pairs per query and page: each launch streams several steps, the candidate buffer is flushed in
    mid-stream, the threshold drops between steps, and the buffer is sorted at its full 2,048 entries"""
    from priblast_amd import capi
    prefix, queries = random_db(ctx, tmp_path)
    queries = queries + ["GGGAAACCCUUUAGCU" * 2]  # a query with fewer pairs than the largest N
    db, qb = open_batch(ctx, prefix, queries)
    try:
        assert db.npages == 3
        opts = capi.default_opts()
        recs = [r for r, _ in summaries(ctx, qb, db, opts)]
        per_page = np.array([np.bincount(r["query"], minlength=len(queries)) for r in recs])  # [page, query]
        assert per_page[:, :6].min() > 2 * K_TOP_TILE, per_page
        assert per_page[:, 6].sum() < 1024, per_page
        for n in (1, 20, 63, 64, 65, 255, 256, 1000, 1024):
            want = rank(recs, n)
            fwd = capi.search_top(ctx, qb, db, n, opts)
            assert_bytes(fwd, want, n)
            rev = capi.search_top(ctx, qb, db, n, opts, pages=[2, 1, 0])
            assert fwd.tobytes() == rev.tobytes(), n
            mid = capi.search_top(ctx, qb, db, n, opts, pages=[1, 2, 0])
            assert fwd.tobytes() == mid.tobytes(), n
    finally:
        qb.close()
        db.close()


def test_top_ties_across_pages(ctx, tmp_path):
    """the same target twice, one copy per page: the two pairs' e_min are bit-identical and the lower page wins"""
    from priblast_amd import capi
    site = "CCACCACACCCAACCACACC"
    comp = site[::-1].translate(str.maketrans("AC", "UG"))
    target = "C" * 30 + site + "C" * 30
    prefix = str(tmp_path / "tiedb")
    capi.db_build(ctx, prefix, ["copy_a", "copy_b", "decoy"], [target, target, "ACGU" * 25], page_size=1)
    db, qb = open_batch(ctx, prefix, ["UUUUUUUUUU" + comp + "UUUUUUUUUU"])
    try:
        assert db.npages == 3
        recs = [r for r, _ in summaries(ctx, qb, db, capi.default_opts())]
        assert len(recs[0]) == 1 and len(recs[1]) == 1
        assert recs[0]["e_min"].view(np.uint64)[0] == recs[1]["e_min"].view(np.uint64)[0]
        assert len(recs[2]) == 0 or recs[2]["e_min"].min() > recs[0]["e_min"][0]  # (the decoy does not win)
        for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
            got = capi.search_top(ctx, qb, db, 1, pages=order)
            assert_bytes(got, rank(recs, 1), order)
            assert int(got[0]["page"]) == 0
            got = capi.search_top(ctx, qb, db, 3, pages=order)
            assert_bytes(got, rank(recs, 3), order)
            assert [int(p) for p in got["page"][:2]] == [0, 1]
    finally:
        qb.close()
        db.close()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "PRB_TRACE_NO_SLOTS=1", "resident=1"])
def test_top_invariance(ctx, golden_dir, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; every final hit re-extended for its base
    pairs; the 3-page database streamed through one resident page: the same bytes"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    prefix = os.path.join(golden_dir, "mixdb")
    db, qb = open_batch(ctx, prefix, seqs)
    try:
        plain = {n: capi.search_top(ctx, qb, db, n) for n in (1, 3)}
    finally:
        qb.close()
        db.close()
    assert sum(len(v) for v in plain.values()) > 10
    name, value = knob.split("=")
    if name != "resident":
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, prefix, seqs, int(value) if name == "resident" else None)
    try:
        for n, want in plain.items():
            assert capi.search_top(ctx, qb, db, n).tobytes() == want.tobytes(), (knob, n)
    finally:
        qb.close()
        db.close()


def test_top_edges(ctx, golden_dir):
    from priblast_amd import capi
    prefix = os.path.join(golden_dir, "mixdb")
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    # a query without hits gives no records
    db, qb = open_batch(ctx, prefix, ["A" * 60])
    try:
        recs, counts = capi.search_top(ctx, qb, db, 5, with_counts=True)
        assert len(recs) == 0 and counts[2] == 0
    finally:
        qb.close()
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    other = capi.QBatch(ctx, seqs[:2], db.repeat_flag)
    other.accessibility(db.W, db.delta)
    try:
        for n in (0, -1, 1025):
            with pytest.raises(capi.PrbError):
                capi.TopSet(ctx, qb, n)
        with capi.TopSet(ctx, qb, 2) as ts:
            ts.merge(db, 1)
            with pytest.raises(capi.PrbError, match="already merged"):
                ts.merge(db, 1)
        # a call refused by the argument checks leaves the table as it was: the page can still be merged
        sums = summaries(ctx, qb, db, capi.default_opts())
        with capi.TopSet(ctx, qb, 2) as ts:
            with pytest.raises(capi.PrbError, match="unsupported option"):
                ts.merge(db, 0, capi.default_opts(drop_out_w_gap=31))
            with pytest.raises(capi.PrbError):
                ts.merge(db, db.npages)
            for p in range(db.npages):
                ts.merge(db, p)
            got = ts.finish()
            assert_bytes(got, rank([r for r, _ in sums], 2), "after refused calls")
            # finished: the device table is gone, a second finish changes nothing, no page can be merged
            assert ts.finish().tobytes() == got.tobytes()
            with pytest.raises(capi.PrbError, match="finished"):
                ts.merge(db, 0)
        with capi.TopSet(ctx, other, 2) as ts:  # a table made for another batch
            with pytest.raises(capi.PrbError, match="another context or query batch"):
                capi._check(capi.lib().prb_search_page_top(ctx.h, qb.h, db.h, 0, ctypes.byref(capi.default_opts()), ts.h))
        # pages left out are simply not in the table
        with capi.TopSet(ctx, qb, 2) as ts:
            ts.merge(db, 2)
            ts.merge(db, 0)
            want = rank([sums[0][0], np.zeros(0, capi.PAIR_DTYPE), sums[2][0]], 2)
            assert_bytes(ts.finish(), want, "pages 0 and 2")
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
    with open(out) as f:
        return f.read()


@pytest.mark.parametrize("tag", ["mix", "quirk"])
def test_cli_top_lines(ctx, golden_dir, tmp_path, tag):
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    full = run_ris(golden_dir, tmp_path, tag, "t.txt", ["-t"]).splitlines()
    tlines = {l.split(",", 1)[1] for l in full[3:]}
    # the C ABI's records ranked in Python, batch by batch as the command line cuts them (longest queries first, 5 a batch)
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
    db = capi.Db(ctx, os.path.join(golden_dir, f"{tag}db"))
    per_batch = []
    try:
        for b0 in range(0, len(order), 5):
            idx = order[b0:b0 + 5]
            qb = capi.QBatch(ctx, [seqs[i] for i in idx], db.repeat_flag)
            qb.accessibility(db.W, db.delta)
            try:
                per_batch.append((idx, [r for r, _ in summaries(ctx, qb, db, capi.default_opts())]))
            finally:
                qb.close()
        for n in (1, 3):
            text = run_ris(golden_dir, tmp_path, tag, f"top{n}.txt", ["-t", "-n", str(n)])
            lines = text.splitlines()
            assert lines[:3] == full[:3]
            body = lines[3:]
            assert [int(l.split(",", 1)[0]) for l in body] == list(range(len(body)))
            assert all(l.split(",", 1)[1] in tlines for l in body)
            want = []
            for idx, recs in per_batch:
                for r in rank(recs, n):
                    want.append((names[idx[int(r["query"])]], db.seq_name(int(r["page"]), int(r["db_id"]))))
            assert [(l.split(",")[1], l.split(",")[3]) for l in body] == want
            assert run_ris(golden_dir, tmp_path, tag, f"two{n}.txt", ["-t", "-n", str(n)], {"PRB_DEVICES": "0,0"}) == text
            assert run_ris(golden_dir, tmp_path, tag, f"s1{n}.txt", ["-t", "-n", str(n), "-s", "1"]) == text
    finally:
        db.close()
