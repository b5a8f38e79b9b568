"""Which launches of a sub-batch's last step are booked to which stage timer, per destination of the final hits: the
hit records and the pair records that go to the host, and every result table.  Only launch counts are compared - they
are integers and the inputs are fixed, so the comparison is exact.

The expected counts were recorded from the library as it was before the search driver got its one emit path
(`python tests/test_gpu_emit_brackets.py` prints them, with the public Python API only, on any commit)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# destination -> the stage of its own bracket (the records' only bracket is the traceback's)
OWN = {"records": "traceback", "summary": "summary", "top": "top", "profile": "profile", "tophits": "tophits", "targets": "targets",
       "coverage": "coverage", "null_observed": "null", "null_decoys": "null", "groups": "group"}
BUDGETS = {"default": None, "one_query": "1"}  # PRB_SEARCH_PAIRS=1: every query a sub-batch of its own

# (budget, destination) -> the launches of ("traceback", "summary", own stage) after page 0 and after all three pages.
# Recorded on commit 026c955 (the parent of the one-emit-path refactor) on an MI355X.
EXPECTED = {
    ("default", "coverage"): ((2, 0, 9), (6, 0, 27)),
    ("default", "groups"): ((2, 3, 3), (6, 9, 9)),
    ("default", "null_decoys"): ((2, 3, 1), (6, 9, 3)),
    ("default", "null_observed"): ((2, 3, 1), (6, 9, 3)),
    ("default", "profile"): ((2, 2, 8), (6, 6, 24)),
    ("default", "records"): ((2, 0, 2), (6, 0, 6)),
    ("default", "summary"): ((2, 3, 3), (6, 9, 9)),
    ("default", "targets"): ((2, 3, 5), (6, 9, 15)),
    ("default", "top"): ((2, 3, 1), (6, 9, 3)),
    ("default", "tophits"): ((2, 0, 4), (6, 0, 12)),
    ("one_query", "coverage"): ((14, 0, 63), (30, 0, 135)),
    ("one_query", "groups"): ((14, 21, 21), (30, 45, 45)),
    ("one_query", "null_decoys"): ((10, 15, 5), (32, 48, 16)),
    ("one_query", "null_observed"): ((14, 21, 7), (30, 45, 15)),
    ("one_query", "profile"): ((14, 14, 56), (30, 30, 120)),
    ("one_query", "records"): ((14, 0, 14), (30, 0, 30)),
    ("one_query", "summary"): ((14, 21, 21), (30, 45, 45)),
    ("one_query", "targets"): ((14, 21, 35), (30, 45, 75)),
    ("one_query", "top"): ((14, 21, 7), (30, 45, 15)),
    ("one_query", "tophits"): ((14, 0, 28), (30, 0, 60)),
}


def open_case(ctx, tmpdir):
    """the `mix` database built in pages of 10 sequences, and its query batch -> (db, qb, query sequences)"""
    import refdump
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    prefix = os.path.join(str(tmpdir), "mixdb")
    capi.db_build(ctx, prefix, names, seqs, 0, 8, 70, 5, 10)
    _, qseqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, prefix)
    qb = capi.QBatch(ctx, qseqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    return db, qb, qseqs


def collect(ctx, db, qb, qseqs):
    """Every destination in turn: reset_timers, every page searched -> {destination: (launches after page 0, launches
    after the last page)}, launches = those of ("traceback", "summary", the destination's own stage)"""
    from priblast_amd import capi
    opts = capi.default_opts()
    ids = np.arange(len(qseqs), dtype=np.int32)
    out = {}

    def run(dest, search):
        ctx.reset_timers()
        rows = []
        for p in range(db.npages):
            search(p)
            if p in (0, db.npages - 1):
                rows.append(tuple(ctx.stage_ms(s)[1] for s in ("traceback", "summary", OWN[dest])))
        out[dest] = tuple(rows)

    run("records", lambda p: capi.search_page(ctx, qb, db, p, opts))
    run("summary", lambda p: capi.search_page_summary(ctx, qb, db, p, opts))
    with capi.TopSet(ctx, qb, 2) as t:
        run("top", lambda p: t.merge(db, p, opts))
    with capi.ProfSet(ctx, qb) as t:
        run("profile", lambda p: t.merge(db, p, opts))
    with capi.TopHits(ctx, qb, 2) as t:
        run("tophits", lambda p: t.merge(db, p, opts))
    with capi.TargetSet(ctx, db, 2) as t:
        run("targets", lambda p: t.merge(qb, p, ids, opts))
    with capi.CovSet(ctx, db) as t:
        run("coverage", lambda p: t.merge(qb, p, ids, opts))
    dseqs, owner, decoy = capi.null_decoys(qseqs, 1)
    dqb = capi.QBatch(ctx, dseqs, db.repeat_flag)
    try:
        dqb.accessibility(db.W, db.delta)
        with capi.NullSet(ctx, qb, db, 1) as t:
            run("null_observed", lambda p: t.observed(p, opts))
            run("null_decoys", lambda p: t.decoys(dqb, p, owner, decoy, opts))
    finally:
        dqb.close()
    maps = [np.arange(db.page_info(p)[0], dtype=np.int32) % 2 for p in range(db.npages)]
    with capi.GroupSet(ctx, qb, db, maps, 2) as t:
        run("groups", lambda p: t.merge(p, opts))
    return out


def collect_budgets(ctx, tmpdir, setenv, delenv):
    db, qb, qseqs = open_case(ctx, tmpdir)
    try:
        assert db.npages == 3
        got = {}
        for budget, pairs in BUDGETS.items():
            if pairs is None:
                delenv("PRB_SEARCH_PAIRS")
            else:
                setenv("PRB_SEARCH_PAIRS", pairs)
            for dest, rows in collect(ctx, db, qb, qseqs).items():
                got[budget, dest] = rows
        return got
    finally:
        delenv("PRB_SEARCH_PAIRS")
        qb.close()
        db.close()


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    from priblast_amd import capi
    mp = pytest.MonkeyPatch()
    try:
        with capi.Context(0) as ctx:
            yield collect_budgets(ctx, tmp_path_factory.mktemp("brackets"), mp.setenv, lambda k: mp.delenv(k, raising=False))
    finally:
        mp.undo()


@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("dest", sorted(OWN))
def test_launches_per_stage_timer(launches, budget, dest):
    print(budget, dest, launches[budget, dest])
    assert launches[budget, dest] == EXPECTED[budget, dest]


def test_summary_bracket_of_one_sub_batch(launches):
    """One page, one sub-batch: the tables that take pair records book the same launches to "summary" - the pair runs
    and the fold -, the profile table one less (no fold), and what takes hits or hit records none."""
    summary = {dest: launches["default", dest][0][1] for dest in OWN}
    print(summary)
    assert summary["top"] == summary["targets"] == summary["null_observed"] == summary["groups"]
    assert summary["top"] == summary["profile"] + 1
    assert summary["records"] == summary["coverage"] == summary["tophits"] == 0


if __name__ == "__main__":
    import pprint
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from priblast_amd import capi
    with capi.Context(0) as c, tempfile.TemporaryDirectory() as d:
        pprint.pprint(collect_budgets(c, d, os.environ.__setitem__, lambda k: os.environ.pop(k, None)), width=120)
