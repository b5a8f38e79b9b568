"""GPU tests of the per-position profile (prb_search_page_profile, `ris -q`): for every query position covered by a final
hit, the number of covering hits, of distinct target sequences among them, their minimum interaction energy and the
first hit in output order that has it, kept in a table on the device that every page of a batch is merged into.  The
yardstick is the contract restated in Python over the hit path (prb_search_page's records and their `-s 0` pairs, which
earlier tests pin to the reference).  The device rows must match it byte for byte."""
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


def hit_path(ctx, qb, db, opts=None, pages=None):
    """[(page, hits, first pair, last pair)] of prb_search_page over the pages, and the summed stage counts"""
    from priblast_amd import capi
    out, counts = [], [0, 0, 0]
    for p in range(db.npages) if pages is None else pages:
        hits, bp, c = capi.search_page(ctx, qb, db, p, opts)
        hits, bp = np.array(hits), np.array(bp)
        off, cnt = hits["bp_offset"].astype(np.int64), hits["bp_count"].astype(np.int64)
        assert (cnt > 0).all()
        out.append((p, hits, bp[off] if len(hits) else np.zeros((0, 2), np.int32),
                    bp[off + cnt - 1] if len(hits) else np.zeros((0, 2), np.int32)))
        counts = [a + int(b) for a, b in zip(counts, c)]
    return out, tuple(counts)


def profile(pages, qlens):
    """The contract restated: pages = hit_path(...)[0] -> PROFILE_DTYPE rows, by query, then position."""
    from priblast_amd import capi
    rows = []
    for q, L in enumerate(qlens):
        sel = []  # this query's hits in output order: page ascending, then place in the page
        for p, hits, first, last in sorted(pages, key=lambda t: t[0]):
            k = np.nonzero(hits["query"] == q)[0]
            for i in k:
                sel.append((p, hits[i], first[i], last[i]))
        if not sel:
            continue
        lo = np.array([min(f[0], l[0]) for _, _, f, l in sel])
        hi = np.array([max(f[0], l[0]) for _, _, f, l in sel])
        assert lo.min() >= 0 and hi.max() < L
        diff = np.zeros(L + 1, np.int64)
        np.add.at(diff, lo, 1)
        np.add.at(diff, hi + 1, -1)
        hits = np.cumsum(diff)[:L]
        # targets: the union of each (page, db_id) pair's spans
        tdiff = np.zeros(L + 1, np.int64)
        spans = {}
        for k, (p, h, _, _) in enumerate(sel):
            spans.setdefault((p, int(h["db_id"])), []).append((int(lo[k]), int(hi[k])))
        for iv in spans.values():
            iv.sort()
            a, b = iv[0]
            for x, y in iv[1:] + [(L + 2, L + 2)]:
                if x > b + 1:
                    tdiff[a] += 1
                    tdiff[b + 1] -= 1
                    a, b = x, y
                else:
                    b = max(b, y)
        targets = np.cumsum(tdiff)[:L]
        # the first hit with the minimum: walked backwards, `<=` lets an earlier hit take a tie (-0.0 == +0.0)
        best_e = np.full(L, np.inf)
        best_i = np.full(L, -1, np.int64)
        e = np.array([float(h["e_tot"]) for _, h, _, _ in sel])
        for k in range(len(sel) - 1, -1, -1):
            seg_e, seg_i = best_e[lo[k]:hi[k] + 1], best_i[lo[k]:hi[k] + 1]
            m = e[k] <= seg_e
            seg_e[m] = e[k]
            seg_i[m] = k
        for pos in np.nonzero(hits > 0)[0]:
            p, h, f, l = sel[best_i[pos]]
            rows.append((q, int(pos), int(hits[pos]), int(targets[pos]), p, int(h["db_id"]), 0, h["e_tot"], f, l))
    out = np.zeros(len(rows), capi.PROFILE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


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


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


def test_profile_equals_hit_path(ctx, golden_dir):
    from priblast_amd import capi
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db, qb = open_batch(ctx, os.path.join(golden_dir, f"{tag}db"), seqs)
        try:
            for kw in OPTS:
                opts = capi.default_opts(**kw)
                pages, counts = hit_path(ctx, qb, db, opts)
                got, got_counts = capi.search_profile(ctx, qb, db, opts, with_counts=True)
                assert got_counts == counts, (tag, kw)
                want = profile(pages, [len(s) for s in seqs])
                assert len(want) > 0, (tag, kw)
                assert_bytes(got, want, (tag, kw))
        finally:
            qb.close()
            db.close()


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "PRB_TRACE_NO_SLOTS=1", "resident=1"])
def test_profile_invariance(ctx, golden_dir, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; every final hit re-extended for its base
    pairs; the 3-page database streamed through one resident page: the same bytes"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    prefix = os.path.join(golden_dir, "mixdb")
    db, qb = open_batch(ctx, prefix, seqs)
    try:
        plain = capi.search_profile(ctx, qb, db)
    finally:
        qb.close()
        db.close()
    assert len(plain) > 10
    name, value = knob.split("=")
    if name != "resident":
        monkeypatch.setenv(name, value)
    db, qb = open_batch(ctx, prefix, seqs, int(value) if name == "resident" else None)
    try:
        assert capi.search_profile(ctx, qb, db).tobytes() == plain.tobytes(), knob
    finally:
        qb.close()
        db.close()


def test_profile_page_order_and_batch(ctx, golden_dir):
    """pages merged reversed or shuffled, and each query searched alone: the same rows"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, "mixdb"), seqs)
    try:
        assert db.npages >= 3
        fwd = capi.search_profile(ctx, qb, db)
        rev = capi.search_profile(ctx, qb, db, pages=list(range(db.npages))[::-1])
        assert fwd.tobytes() == rev.tobytes()
        order = list(np.random.default_rng(5).permutation(db.npages))
        assert capi.search_profile(ctx, qb, db, pages=[int(p) for p in order]).tobytes() == fwd.tobytes()
    finally:
        qb.close()
    try:
        for q, s in enumerate(seqs):
            one = capi.QBatch(ctx, [s], db.repeat_flag)
            one.accessibility(db.W, db.delta)
            try:
                alone = capi.search_profile(ctx, one, db)
            finally:
                one.close()
            want = fwd[fwd["query"] == q].copy()
            want["query"] = 0
            assert alone.tobytes() == want.tobytes(), q
    finally:
        db.close()


def test_profile_ties_and_distinct_targets(ctx, tmp_path):
    """one target three times, twice in page 0 and once in page 1, each copy with the query's site twice: the minima tie
    within and across pages and the first copy's first hit wins; Targets counts the three copies, never a pair twice"""
    from priblast_amd import capi
    site = "CCACCACACCCAACCACACC"
    comp = site[::-1].translate(str.maketrans("AC", "UG"))
    target = "C" * 30 + site + "C" * 40 + site + "C" * 30
    prefix = str(tmp_path / "tiedb")
    capi.db_build(ctx, prefix, ["copy_a", "copy_b", "copy_c", "decoy"], [target, target, target, "ACGU" * 25], page_size=2)
    seqs = ["UUUUUUUUUU" + comp + "UUUUUUUUUU"]
    db, qb = open_batch(ctx, prefix, seqs)
    try:
        assert db.npages == 2
        pages, _ = hit_path(ctx, qb, db)
        per_seq = {}
        for p, hits, _, _ in pages:
            for h in hits:
                per_seq[(p, int(h["db_id"]))] = per_seq.get((p, int(h["db_id"])), 0) + 1
        assert per_seq.get((0, 0), 0) >= 2 and per_seq.get((0, 1)) == per_seq[(0, 0)] == per_seq.get((1, 0))
        want = profile(pages, [len(seqs[0])])
        for order in ([0, 1], [1, 0]):
            got = capi.search_profile(ctx, qb, db, pages=order)
            assert_bytes(got, want, order)
        assert (got["page"] == 0).all() and (got["db_id"] == 0).all()
        assert got["targets"].max() == 3
        assert (got["hits"] > got["targets"]).any()  # two hits of one pair on a position: one target
    finally:
        qb.close()
        db.close()


def test_profile_long_query_and_hot_position(ctx, tmp_path):
    """a 13 kb query beyond any tile of positions, and a site that thousands of targets share: one position covered
    by thousands of hits"""
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    site = "CCACCACACCCAACCACACC"
    comp = site[::-1].translate(str.maketrans("AC", "UG"))
    targets = [random_seq(rng, 40) + site + random_seq(rng, 40) for _ in range(2500)]
    targets += [random_seq(rng, 500) for _ in range(300)]
    prefix = str(tmp_path / "hotdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(targets))], targets, page_size=1000)
    seqs = [random_seq(rng, 13000), random_seq(rng, 300) + comp + random_seq(rng, 300)]
    db, qb = open_batch(ctx, prefix, seqs)
    try:
        pages, _ = hit_path(ctx, qb, db)
        want = profile(pages, [len(s) for s in seqs])
        got = capi.search_profile(ctx, qb, db)
        assert_bytes(got, want, "long and hot")
        assert got[got["query"] == 0]["pos"].max() > 12000
        assert got["hits"].max() >= 2000 and got["targets"].max() >= 2000
    finally:
        qb.close()
        db.close()


def test_profile_edges(ctx, golden_dir):
    from priblast_amd import capi
    prefix = os.path.join(golden_dir, "mixdb")
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    # a query without hits gives no rows
    db, qb = open_batch(ctx, prefix, ["A" * 60])
    try:
        rows, counts = capi.search_profile(ctx, qb, db, with_counts=True)
        assert len(rows) == 0 and counts[2] == 0
    finally:
        qb.close()
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    other = capi.QBatch(ctx, seqs[:2], db.repeat_flag)
    other.accessibility(db.W, db.delta)
    ctx2 = capi.Context(0)
    try:
        want = capi.search_profile(ctx, qb, db)
        with capi.ProfSet(ctx, qb) as ps:
            ps.merge(db, 1)
            with pytest.raises(capi.PrbError, match="already merged"):
                ps.merge(db, 1)
        # calls refused by the argument checks leave the table as it was
        with capi.ProfSet(ctx, qb) as ps:
            with pytest.raises(capi.PrbError, match="unsupported option"):
                ps.merge(db, 0, capi.default_opts(drop_out_w_gap=31))
            with pytest.raises(capi.PrbError):
                ps.merge(db, db.npages)
            with pytest.raises(capi.PrbError):
                ps.merge(db, -1)
            with pytest.raises(capi.PrbError, match="another context or query batch"):
                capi._check(capi.lib().prb_search_page_profile(ctx.h, other.h, db.h, 0, ctypes.byref(capi.default_opts()), ps.h))
            with pytest.raises(capi.PrbError):
                capi._check(capi.lib().prb_search_page_profile(ctx2.h, qb.h, db.h, 0, ctypes.byref(capi.default_opts()), ps.h))
            with pytest.raises(capi.PrbError):
                capi._check(capi.lib().prb_profset_finish(ctx2.h, ps.h))
            for p in range(db.npages):
                ps.merge(db, p)
            got = ps.finish()
            assert_bytes(got, want, "after refused calls")
            # finished: the device table is gone, a second finish changes nothing, no page can be merged
            assert ps.finish().tobytes() == got.tobytes()
            with pytest.raises(capi.PrbError, match="finished"):
                ps.merge(db, 0)
            assert ps.finish().tobytes() == got.tobytes()
        # the formatter takes the rows (and refuses rows out of order)
        names = [f"q{i}" for i in range(len(seqs))]
        ql = [qb.length_unmasked(i) for i in range(len(seqs))]
        lines, nbytes = capi.write_profile_lines(db, names, ql, want)
        assert lines == len(want) and nbytes > 0
        if len(want) > 1:
            with pytest.raises(capi.PrbError, match="inconsistent"):
                capi.write_profile_lines(db, names, ql, want[::-1])
    finally:
        qb.close()
        other.close()
        db.close()
        ctx2.close()


def run_ris(golden_dir, tmp_path, tag, name, extra=(), env_extra=None):
    from priblast_amd import capi
    out = str(tmp_path / name)
    env = dict(os.environ, PRB_BATCH="5")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    env.update(env_extra or {})
    subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, f"{tag}_q.fa"), "-o", out, "-d",
                    os.path.join(golden_dir, f"{tag}db")] + list(extra), check=True, env=env, timeout=600)
    with open(out) as f:
        return f.read()


def span_of(bp_field):
    """'(q0-qN:t0-tN) ' -> (lo, hi) of the query side"""
    q = bp_field.strip()[1:-1].split(":")[0]
    a, b = (int(x) for x in q.split("-"))
    return min(a, b), max(a, b)


@pytest.mark.parametrize("tag", ["mix", "quirk"])
def test_cli_profile_lines(golden_dir, tmp_path, tag):
    text = run_ris(golden_dir, tmp_path, tag, "q.txt", ["-q"])
    lines = text.splitlines()
    full = run_ris(golden_dir, tmp_path, tag, "full.txt").splitlines()
    assert lines[:2] == full[:2]
    assert lines[2] == ("Id,Query name,Query Length,Position,Hits,Targets,Minimum Interaction Energy,Target name,"
                        "Target Length,BasePair")
    body = [l.split(",") for l in lines[3:]]
    assert [int(f[0]) for f in body] == list(range(len(body)))
    got = {(f[1], int(f[3])): f for f in body}
    assert len(got) == len(body)
    # the reference's own result lines: qname,qlen,dbname,dblen,Eacc,Ehyb,Etot,BasePair
    with open(os.path.join(GOLDEN, f"{tag}_ris_s0.out")) as fh:
        ref = [l.rstrip("\n").split(",") for l in fh.read().splitlines()[2:] if l.strip()]
    # this build's own result lines, in output order, for the first of tied minima
    own = [l.split(",")[1:] for l in full[3:]]
    cover = {}
    for f in ref:
        lo, hi = span_of(f[7])
        for p in range(lo, hi + 1):
            cover.setdefault((f[0], p), []).append(f)
    own_cover = {}
    for f in own:
        lo, hi = span_of(f[7])
        for p in range(lo, hi + 1):
            own_cover.setdefault((f[0], p), []).append(f)
    assert set(got) == set(cover)
    for key, fs in cover.items():
        g = got[key]
        assert g[2] == fs[0][1]  # Query Length as the result lines print it
        assert int(g[4]) == len(fs), key
        assert int(g[5]) == len({f[2] for f in fs}), key
        emin = min(float(f[6]) for f in fs)
        best = [f for f in fs if float(f[6]) == emin]
        assert g[6] == best[0][6], key
        if len(best) == 1:
            assert g[7:] == best[0][2:4] + best[0][7:], key
        else:
            mine = [f for f in own_cover[key] if float(f[6]) == emin]
            assert g[7:] == mine[0][2:4] + mine[0][7:], key
    assert len(cover) > 20
    # the same file with two workers on one GPU, with -s 1, and with one query per batch
    assert run_ris(golden_dir, tmp_path, tag, "two.txt", ["-q"], {"PRB_DEVICES": "0,0"}) == text
    assert run_ris(golden_dir, tmp_path, tag, "s1.txt", ["-q", "-s", "1"]) == text
    assert run_ris(golden_dir, tmp_path, tag, "b1.txt", ["-q"], {"PRB_BATCH": "1"}) == text
