"""GPU tests of the per-target table (prb_search_page_targets, `ris -r N`): each target's N pairs of lowest minimum
interaction energy over all the queries merged in, kept in a table on the device.  The yardstick is the per-pair
summary search over every batch and page (pinned to the hit path by test_gpu_summary.py), ranked here in Python: per
(page, db_id) the records in query-identifier order, stable-sorted by e_min, cut to N.  The table must match it byte
for byte."""
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


def rank(calls, n):
    """The contract restated: calls = [(ids, page, PAIR_DTYPE records of that batch against that page)] -> TARGET_DTYPE
    records by page, db_id and rank."""
    from priblast_amd import capi
    per_t = {}
    for ids, page, recs in calls:
        for r in recs:
            per_t.setdefault((page, int(r["db_id"])), []).append((int(ids[int(r["query"])]), r))
    chosen = []
    for key in sorted(per_t):
        by_id = sorted(per_t[key], key=lambda t: t[0])
        ranked = sorted(by_id, key=lambda t: float(t[1]["e_min"]))  # stable: ties by identifier (-0.0 == +0.0)
        chosen += [(key[0], k, qid, r) for k, (qid, r) in enumerate(ranked[:n])]
    out = np.zeros(len(chosen), capi.TARGET_DTYPE)
    for i, (p, k, qid, r) in enumerate(chosen):
        for f in capi.PAIR_DTYPE.names:
            out[i][f] = r[f]
        out[i]["query"], out[i]["page"], out[i]["rank"] = qid, p, k
    return out


def most_per_target(calls):
    count = {}
    for _, page, recs in calls:
        for d in recs["db_id"]:
            count[(page, int(d))] = count.get((page, int(d)), 0) + 1
    return max(count.values()) if count else 1


def open_batch(ctx, db, seqs):
    from priblast_amd import capi
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    return qb


def summaries(ctx, qb, db, ids, opts=None):
    """-> ([(ids, page, records)], summed counts)"""
    from priblast_amd import capi
    got = [capi.search_page_summary(ctx, qb, db, p, opts, with_counts=True) for p in range(db.npages)]
    return [(ids, p, r) for p, (r, _) in enumerate(got)], tuple(int(sum(c[i] for _, c in got)) for i in range(3))


def assert_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    """the mix database (3 pages), its queries as one batch with identifiers 0..nq-1, and their summaries (computed once)"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
    qb = open_batch(ctx, db, seqs)
    ids = np.arange(len(seqs), dtype=np.int32)
    calls, counts = summaries(ctx, qb, db, ids)

    class Mix:
        pass
    m = Mix()
    m.names, m.seqs, m.db, m.qb, m.ids, m.calls, m.counts = names, seqs, db, qb, ids, calls, counts
    yield m
    qb.close()
    db.close()


def test_targets_equal_ranked_summaries(ctx, golden_dir):
    from priblast_amd import capi
    cut = 0
    for tag in ("c1", "mix", "quirk"):
        _, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        db = capi.Db(ctx, os.path.join(golden_dir, f"{tag}db"))
        qb = open_batch(ctx, db, seqs)
        ids = np.arange(len(seqs), dtype=np.int32)
        try:
            for kw in OPTS:
                opts = capi.default_opts(**kw)
                calls, counts = summaries(ctx, qb, db, ids, opts)
                most = most_per_target(calls)
                for n in (1, 2, 3, most, most + 5):
                    got, got_counts = capi.search_targets(ctx, db, n, [(qb, ids)], opts, with_counts=True)
                    assert got_counts == counts
                    want = rank(calls, n)
                    assert_bytes(got, want, (tag, kw, n))
                    cut += len(want) < sum(len(r) for _, _, r in calls)
        finally:
            qb.close()
            db.close()
    assert cut > 0


def test_targets_do_not_depend_on_batching_or_order(ctx, mix, monkeypatch):
    """one batch; three batches forward and in reverse with identifiers that are a permutation; the pages in reverse; every
    query a sub-batch of its own: the same bytes"""
    from priblast_amd import capi
    db, seqs = mix.db, mix.seqs
    nq = len(seqs)
    perm = np.random.default_rng(11).permutation(nq).astype(np.int32)
    assert not np.array_equal(perm, np.arange(nq))
    cuts = [0, nq // 3, 2 * nq // 3, nq]
    parts = [list(range(cuts[k], cuts[k + 1])) for k in range(3)]
    batches = [(open_batch(ctx, db, [seqs[i] for i in part]), perm[part]) for part in parts]
    try:
        # the yardstick with the permuted identifiers: the one batch's summaries, renamed
        calls = [(perm, p, r) for _, p, r in mix.calls]
        for n in (2, 1000):
            want = rank(calls, n)
            one = capi.search_targets(ctx, db, n, [(mix.qb, perm)])
            assert_bytes(one, want, ("one batch", n))
            assert capi.search_targets(ctx, db, n, batches).tobytes() == one.tobytes(), n
            assert capi.search_targets(ctx, db, n, batches[::-1]).tobytes() == one.tobytes(), n
            assert capi.search_targets(ctx, db, n, batches, pages=list(range(db.npages))[::-1]).tobytes() == one.tobytes(), n
            monkeypatch.setenv("PRB_SEARCH_PAIRS", "1")
            assert capi.search_targets(ctx, db, n, [(mix.qb, perm)]).tobytes() == one.tobytes(), n
            monkeypatch.delenv("PRB_SEARCH_PAIRS")
    finally:
        for qb, _ in batches:
            qb.close()


def test_targets_ties_go_by_identifier(ctx, mix):
    """the same query sequence under two identifiers, in different batches, the higher one merged first: bit-identical
    e_min in every target the query has, the two records adjacent and in identifier order"""
    from priblast_amd import capi
    db, nq = mix.db, len(mix.seqs)
    best = int(np.bincount(np.concatenate([r["query"] for _, _, r in mix.calls]), minlength=nq).argmax())
    twin_id = nq + 5
    twin = open_batch(ctx, db, [mix.seqs[best]])
    try:
        twin_ids = np.array([twin_id], np.int32)
        got = capi.search_targets(ctx, db, 1000, [(twin, twin_ids), (mix.qb, mix.ids)])
        twin_calls, _ = summaries(ctx, twin, db, twin_ids)
        assert_bytes(got, rank(mix.calls + twin_calls, 1000), "twin")
        at = np.flatnonzero(got["query"] == twin_id)
        assert len(at) > 0
        for i in at:
            a, b = got[i - 1], got[i]
            assert (int(a["query"]), int(a["page"]), int(a["db_id"])) == (best, int(b["page"]), int(b["db_id"]))
            assert a["e_min"].tobytes() == b["e_min"].tobytes() and int(b["rank"]) == int(a["rank"]) + 1
    finally:
        twin.close()


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


def test_targets_long_runs(ctx, tmp_path, monkeypatch):
    """40 random 500-nt targets and 150 random 2-kb queries in one batch and one sub-batch: nearly every pair has a final
    hit, so a target's run in the sub-batch is longer than two steps of 64 records - several steps of k_target_merge with
    the threshold lowered in between, and slots handed on from one step to the next"""
    from priblast_amd import capi
    rng = np.random.default_rng(5)
    targets = [random_seq(rng, 500) for _ in range(40)]
    prefix = str(tmp_path / "longdb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(targets))], targets)
    queries = [random_seq(rng, 2000) for _ in range(150)]
    ids = rng.permutation(len(queries)).astype(np.int32)
    monkeypatch.setenv("PRB_SEARCH_PAIRS", "1e15")  # (the whole batch is one sub-batch)
    db = capi.Db(ctx, prefix)
    qb = open_batch(ctx, db, queries)
    try:
        calls, counts = summaries(ctx, qb, db, ids)
        assert most_per_target(calls) > 128, most_per_target(calls)
        for n in (1, 63, 64, 65, 128, 1024):
            got, got_counts = capi.search_targets(ctx, db, n, [(qb, ids)], with_counts=True)
            assert got_counts == counts
            assert_bytes(got, rank(calls, n), n)
    finally:
        qb.close()
        db.close()


def test_targetset_merge(ctx, mix, golden_dir):
    from priblast_amd import capi
    db, seqs = mix.db, mix.seqs
    nq = len(seqs)
    half = nq // 2
    a_ids, b_ids = mix.ids[:half], mix.ids[half:]
    qa, qbb = open_batch(ctx, db, seqs[:half]), open_batch(ctx, db, seqs[half:])
    other_db = capi.Db(ctx, os.path.join(golden_dir, "c1db"))
    try:
        def fill(n, which):
            """a table over the (batch, page) sets `which`"""
            ts = capi.TargetSet(ctx, db, n)
            for qb, ids, page in which:
                ts.merge(qb, page, ids)
            return ts
        left = [(qa, a_ids, 0), (qa, a_ids, 1), (qa, a_ids, 2), (qbb, b_ids, 0)]
        right = [(qbb, b_ids, 2), (qbb, b_ids, 1)]
        for n in (2, 1000):
            want = rank(mix.calls, n)
            for first, second in ((left, right), (right, left)):
                with fill(n, first) as dst, fill(n, second) as src:
                    dst.absorb(src)
                    assert dst.counts() == mix.counts
                    assert_bytes(dst.finish(), want, ("merged", n))
                    assert src.counts() == (0, 0, 0) and len(src.finish()) == 0
        # refused merges leave both tables as they were
        want = rank(mix.calls, 2)
        with fill(2, left) as dst, fill(2, right) as src:
            with fill(2, right[:1]) as overlap, pytest.raises(capi.PrbError, match="both"):
                src.absorb(overlap)
            with fill(3, []) as other_n, pytest.raises(capi.PrbError, match="records per target"):
                dst.absorb(other_n)
            with capi.TargetSet(ctx, other_db, 2) as foreign, pytest.raises(capi.PrbError, match="different databases"):
                dst.absorb(foreign)
            with pytest.raises(capi.PrbError):
                dst.absorb(dst)
            dst.absorb(src)
            assert_bytes(dst.finish(), want, "after refused merges")
            with fill(2, []) as late, pytest.raises(capi.PrbError, match="finished"):
                late.absorb(dst)
    finally:
        qa.close()
        qbb.close()
        other_db.close()


def test_targets_argument_refusals(ctx, mix, golden_dir):
    from priblast_amd import capi
    db, nq = mix.db, len(mix.seqs)
    other_db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))  # the same files under another handle
    try:
        for n in (0, -1, 1025):
            with pytest.raises(capi.PrbError):
                capi.TargetSet(ctx, db, n)
        with capi.TargetSet(ctx, db, 2) as ts:
            ts.merge(mix.qb, 1, mix.ids)
            twice = mix.ids.copy()
            twice[1] = twice[0]
            shifted = mix.ids + nq  # fresh identifiers but for the one that is repeated below
            for bad, page, why in ((twice + nq, 0, "twice"), (mix.ids, 1, "already merged"), (-1 - mix.ids, 0, "below 0"),
                                   (np.where(mix.ids == 3, 3, shifted), 1, "already merged")):
                with pytest.raises(capi.PrbError, match=why):
                    ts.merge(mix.qb, page, bad)
            with pytest.raises(capi.PrbError, match="another database"):
                ts.merge(mix.qb, 0, mix.ids, db=other_db)
            with pytest.raises(capi.PrbError, match="distinct_sites"):
                ts.merge(mix.qb, 0, mix.ids, capi.default_opts(distinct_sites=1))
            with pytest.raises(capi.PrbError, match="unsupported option"):
                ts.merge(mix.qb, 0, mix.ids, capi.default_opts(drop_out_w_gap=31))
            ts.merge(mix.qb, 2, mix.ids)
            ts.merge(mix.qb, 0, mix.ids)
            got = ts.finish()
            assert_bytes(got, rank(mix.calls, 2), "after refused calls")
            assert ts.finish().tobytes() == got.tobytes()
            with pytest.raises(capi.PrbError, match="finished"):
                ts.merge(mix.qb, 0, mix.ids + nq)
    finally:
        other_db.close()


def run_ris(golden_dir, tmp_path, name, extra=(), env_extra=None):
    from priblast_amd import capi
    out = str(tmp_path / name)
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", out, "-d", os.path.join(golden_dir, "mixdb")] +
                   list(extra), check=True, env=env, timeout=600)
    with open(out, "rb") as f:
        return f.read()


RUNS = {"plain": {}, "batch_1": {"PRB_BATCH": "1"}, "two_workers": {"PRB_DEVICES": "0,0"},
        "page_team": {"PRB_DEVICES": "0,0,0", "PRB_SPLIT": "pages"}, "one_resident_page": {"PRB_DB_RESIDENT_PAGES": "1"}}


@pytest.mark.parametrize("distinct", [False, True], ids=["all_hits", "distinct_sites"])
def test_cli_target_lines(ctx, mix, golden_dir, tmp_path, distinct):
    from priblast_amd import capi
    u = ["-u"] if distinct else []
    opts = capi.default_opts(distinct_sites=1 if distinct else 0)
    full = run_ris(golden_dir, tmp_path, "t.txt", ["-t"] + u).decode().splitlines(keepends=True)
    header, tbody = full[:3], [l.split(",", 1)[1] for l in full[3:]]
    per_target = {}
    for l in tbody:
        per_target[l.split(",")[2]] = per_target.get(l.split(",")[2], 0) + 1
    qlen = [mix.qb.length_unmasked(q) for q in range(len(mix.seqs))]
    for n in (2, 1000):
        recs = capi.search_targets(ctx, mix.db, n, [(mix.qb, mix.ids)], opts)
        ref = tmp_path / f"ref{n}.txt"
        fd = os.open(str(ref), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        try:
            os.write(fd, "".join(header).encode())
            lines, _ = capi.write_target_lines(mix.db, mix.names, qlen, recs, fd=fd)
        finally:
            os.close(fd)
        assert lines == len(recs)
        want = ref.read_bytes()
        for name, env in RUNS.items():
            if distinct and name not in ("plain", "page_team"):
                continue
            assert run_ris(golden_dir, tmp_path, f"r{n}_{name}.txt", ["-r", str(n)] + u, env) == want, (n, name)
        body = want.decode().splitlines(keepends=True)[3:]
        assert [int(l.split(",", 1)[0]) for l in body] == list(range(len(body)))
        assert set(l.split(",", 1)[1] for l in body) <= set(tbody)
        got_per_target = {}
        for l in body:
            got_per_target[l.split(",")[3]] = got_per_target.get(l.split(",")[3], 0) + 1
        assert got_per_target == {t: min(n, c) for t, c in per_target.items()}
