"""The front gapped kernel (gapped_front.hip) against the LDS tiers alone (PRB_GAPPED_FRONT=0), as
test_gpu_search.py::test_fallback_kernels_match_tier1 compares them, on inputs made for what the kernel's prologue and
candidate scan do: the accessibility terms of a direction are all loaded at once (a term that is not there, and every term
of a lane beyond the list's end, from a place of its own), the next tile comes from a work counter, and a cell reads its
direction's records in batches of eight.  Equality is exact: counts, hit records and base pairs.

Every input was designed on the CPU: the database built by the reference's `db`, the stages by the oracle port
(tests/oraclelib.py, Db.stages).  CASES holds, per case, the oracle's (seeds, post-ungapped hits, final hits) and the number
of launches of the front kernel; the test asserts them, so that a change of the generator or of the seeds cannot silently
turn a case into another one.  The random short sequences and the wobble duplex bind too weakly for the default final
threshold (-8 kcal/mol; their hits have -3.7 .. -7.9), and a search returns final hits only: the tile_N (N <= 65) and
wobble cases run with final_threshold = 0 - both searches, and the oracle -, under which every post-ungapped hit of theirs
is a final hit whose fields and base pairs are compared (tile_32: 32 hits with 256 pairs).

* tile_N: one 200 nt query (gen_synthetic, seed 11) against a choice of 60 nt sequences (seed 12) with exactly N
  post-ungapped hits: 1, 32 (a full tile of the first launch), 33 (a tile and one hit), 64 and 65.  short_db_N (N
  sequences of 40 nt, the query the reverse complement of the first and the last): hits at the first position of the first
  and at the last position of the last sequence of the page, 2 / 3 / 22 hits.
* tile_grid: ntiles = grid + 1, the smallest list whose last tile comes from the work counter.  The grid is 2,048
  wavefronts (256 compute units x 8), so that takes 65,537 .. 65,568 hits of one query: a 2 kb query (seed 21) against
  1 kb sequences (seed 22) with 60 nt sequences (seed 23) behind them to land inside that window: 65,541 hits, 2,049 tiles
  in the first launch.
* dense_gc, dense_gc2: a query and a target that are reverse complements of each other over (GGGCCC)20 / (GGGCCC)40:
  around every hit most cells of every anti-diagonal are filled.  The developer build's counters (make prof; the ones
  tools/front_profile.py prints; tools/front_cases_profile.py runs these cases under them) on an MI355X, first and second launch together: dense_gc 404 cells, the scan of 254 takes a
  second batch (more than 8 records), of 98 a third (more than 16), 8 directions given up for an improvement; dense_gc2
  1,450 cells, 536 / 65, 97 given up.  Neither fills a direction's 24 records or outgrows the step's cell list; tile_grid
  does (1,234,049 cells: second batch 293,189, third 23,821, 113 cells of a direction with 23 records, 35 directions given
  up for more than 24 cells, 5 steps that outgrow the cell list or the pool, 12,837 given up for an improvement), with the
  work counter handing out tiles meanwhile.
* wobble: (GGGCCC)12 against its reverse complement with every third pair of the duplex a G-U wobble pair where the target
  has a G or a U ((GU)n against (GU)n gives no seed, and two wobble pairs in a row end a helix, so pure G-U stretches fill
  no cell).  One hit (6 pairs), 44 cells, 8 of them behind a wobble pair (the W1 / W2 masks), the scan of 10 in its third batch.  The tile_N
  cases have wobble pairs too (92 of the 397 cells of tile_32, 256,795 in tile_grid).
* the second launch (a lane per hit, 64 hits per tile): on the C1 and quirk goldens (every page, also against the committed
  reference stages) and on every synthetic case that hands hits over, asserted through the launch count; in dense_gc its list is shorter than 64.  PRB_GAPPED_FRONT_PAIRED and
  PRB_GAPPED_HANDOVER=0 once each on dense_gc2: the other instantiation of the second launch, the other caller.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gen_synthetic  # noqa: E402
import refdump  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID = 2048  # wavefronts of a launch of the front kernel: 256 compute units x 8


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


COMP = {"A": "U", "C": "G", "G": "C", "U": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def dense(n):
    t = "GGGCCC" * n
    return [revcomp(t)], ["t0"], [t]


def wobble():
    t = "GGGCCC" * 12
    q = []
    for k, c in enumerate(reversed(t)):
        q.append({"G": "U", "U": "G"}[c] if c in "GU" and k % 3 == 0 else COMP[c])
    return ["".join(q)], ["t0"], [t]


def short_db(nseq):
    recs = list(gen_synthetic.gen(nseq, 40, 7, "s"))
    seqs = [r[1] for r in recs]
    q = revcomp(seqs[0]) + "A" * 5 + revcomp(seqs[-1])
    return [q], [r[0] for r in recs], seqs


# the sequences of gen(400, 60, 12) kept, taken in order while they fit (trimmed sequence by sequence on the oracle's counts)
TILE_KEEP = {
    1: [1],
    32: [0, 1, 2, 4, 5, 6, 7, 8, 10, 12, 14, 15, 16, 18, 19, 20, 22, 23],
    33: [0, 1, 2, 4, 5, 6, 7, 8, 10, 12, 14, 15, 16, 18, 19, 20, 22, 23, 37],
    64: [0, 1, 2, 4, 5, 6, 7, 8, 10, 12, 14, 15, 16, 18, 19, 20, 22, 23, 24, 25, 26, 27, 30, 32, 35, 36, 37, 38, 39, 41, 42, 43,
         44, 45, 49, 50],
    65: [0, 1, 2, 4, 5, 6, 7, 8, 10, 12, 14, 15, 16, 18, 19, 20, 22, 23, 24, 25, 26, 27, 30, 32, 35, 36, 37, 38, 39, 41, 42, 43,
         44, 45, 46],
}


def tile(n):
    q = next(gen_synthetic.gen(1, 200, 11, "q"))[1]
    recs = list(gen_synthetic.gen(400, 60, 12, "s"))
    return [q], [recs[i][0] for i in TILE_KEEP[n]], [recs[i][1] for i in TILE_KEEP[n]]


TILE_GRID_KEEP = (291, (0, 1))  # the first 291 sequences of 1 kb and two of 60 nt: 65,520 + 21 hits by the oracle


def tile_grid():
    q = next(gen_synthetic.gen(1, 2000, 21, "q"))[1]
    big, small = TILE_GRID_KEEP
    recs = list(gen_synthetic.gen(330, 1000, 22, "b"))[:big]
    tail = list(gen_synthetic.gen(150, 60, 23, "t"))
    recs += [tail[i] for i in small]
    return [q], [r[0] for r in recs], [r[1] for r in recs]


# case: (inputs, the oracle's (seeds, post-ungapped hits, final hits), launches of the front kernel[, final_threshold])
CASES = {
    "tile_1": (lambda: tile(1), (12, 1, 1), 1, 0.0),
    "tile_32": (lambda: tile(32), (188, 32, 32), 2, 0.0),
    "tile_33": (lambda: tile(33), (190, 33, 33), 2, 0.0),
    "tile_64": (lambda: tile(64), (313, 64, 64), 2, 0.0),
    "tile_65": (lambda: tile(65), (316, 65, 65), 2, 0.0),
    "tile_grid": (tile_grid, (573530, 65541, 1865), 2),
    "short_db_1": (lambda: short_db(1), (68, 2, 2), 1),
    "short_db_3": (lambda: short_db(3), (74, 3, 2), 1),
    "short_db_40": (lambda: short_db(40), (143, 22, 3), 2),
    "dense_gc": (lambda: dense(20), (40, 10, 3), 2),
    "dense_gc2": (lambda: dense(40), (532, 50, 18), 2),
    "wobble": (wobble, (12, 1, 1), 1, 0.0),
}


def search_both(ctx, qb, db, monkeypatch, env, page=0, **opts):
    """-> (counts, launches of the front kernel) of the search with the front kernel, after comparing it with the tiers alone"""
    from priblast_amd import capi
    settings = [e.partition("=")[::2] for e in env.split(",") if e]
    try:
        monkeypatch.setenv("PRB_GAPPED_FRONT", "0")
        h0, bp0, c0 = capi.search_page(ctx, qb, db, page, capi.default_opts(output_style=1, **opts))
        monkeypatch.delenv("PRB_GAPPED_FRONT")
        for name, value in settings:
            monkeypatch.setenv(name, value or "1")
        ctx.reset_timers()
        h1, bp1, c1 = capi.search_page(ctx, qb, db, page, capi.default_opts(output_style=1, **opts))
        launches = ctx.stage_ms("gapped_front")[1]
        assert c0 == c1
        assert np.array_equal(h0, h1) and np.array_equal(bp0, bp1)
        assert len(h1) == c1[2] and (len(h1) == 0 or len(bp1) > 0)  # (what was compared: every final hit, with its pairs)
        return tuple(c1), launches, h1, bp1
    finally:
        for name, _ in settings:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.delenv("PRB_GAPPED_FRONT", raising=False)


def run(ctx, tmp_path, monkeypatch, case, env=""):
    from priblast_amd import capi
    qs, names, seqs = CASES[case][0]()
    opts = {"final_threshold": CASES[case][3]} if len(CASES[case]) > 3 else {}
    prefix = str(tmp_path / "db")
    capi.db_build(ctx, prefix, names, seqs, 0, 8, 70, 5)
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, qs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    try:
        counts, launches, _, _ = search_both(ctx, qb, db, monkeypatch, env, **opts)
        print(case, env, "counts", counts, "front launches", launches)
        return counts, launches
    finally:
        qb.close()
        db.close()


@pytest.mark.parametrize("case", list(CASES))
def test_front_kernel_matches_tiers(ctx, tmp_path, monkeypatch, case):
    counts, launches = run(ctx, tmp_path, monkeypatch, case)
    assert counts == CASES[case][1]
    assert counts[2] > 0  # (a case without final hits compares nothing)
    assert launches == CASES[case][2]


@pytest.mark.parametrize("env", ["PRB_GAPPED_FRONT_PAIRED", "PRB_GAPPED_HANDOVER=0"])
def test_front_kernel_other_callers_dense(ctx, tmp_path, monkeypatch, env):
    """the other instantiation of the second launch (two launches still), and the cascade without the hand-over (one)"""
    counts, launches = run(ctx, tmp_path, monkeypatch, "dense_gc2", env)
    assert counts == CASES["dense_gc2"][1]
    assert launches == (2 if env == "PRB_GAPPED_FRONT_PAIRED" else 1)


@pytest.mark.parametrize("tag", ["c1", "quirk"])
def test_second_launch_on_goldens(ctx, golden_dir, monkeypatch, tag):
    """the goldens send hits through the hand-over: on every page the search with the front kernel equals the tiers alone and
    the committed reference stages, and the second launch (a lane per hit) runs"""
    from priblast_amd import capi
    from test_gpu_search import as_dicts, key, same
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    stg = refdump.read_stages(os.path.join(golden_dir, f"{tag}.stg"))
    db = capi.Db(ctx, os.path.join(golden_dir, f"{tag}db"))
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    try:
        most = total = 0
        for page in range(db.npages):
            counts, launches, hits, bp = search_both(ctx, qb, db, monkeypatch, "", page=page)
            print(tag, "page", page, "counts", counts, "front launches", launches)
            most = max(most, launches)
            mine = as_dicts(hits, bp)
            nref = 0
            for rec in stg:
                if rec["page"] != page:
                    continue
                got = sorted((h for h in mine if h["query"] == rec["q"]), key=key)
                assert len(got) == len(rec["gapped"]), (page, rec["q"])
                for a, b in zip(got, sorted(rec["gapped"], key=key)):
                    assert same(a, b), (page, rec["q"], a, b)
                nref += len(got)
            assert nref == len(mine)
            total += nref
        assert total > 0 and most >= 2
    finally:
        qb.close()
        db.close()
