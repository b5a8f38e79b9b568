"""Tier 0's pooled fill (the filled cells of a pair step dealt over the whole wavefront) against the per-group fill
(PRB_GAPPED_POOL=0) and the oracle, on batches whose hits are deliberately unequal: dense GC-rich and alternating-GC
duplexes, whose extensions fill many cells per anti-diagonal, mixed with random sequences whose hits find next to
nothing, so that the groups of a wavefront bring very different numbers of cells to each step.  With PRB_GAPPED_FRONT=0
every hit goes through tier 0.  Drop-out lengths -x 1 (everything older than the last anti-diagonal pruned: the B cells
of a pair step fall back to A's first cell as their default predecessor), 16 and 30, minimum helix lengths -m 1, 3 and 7.
The alternating-GC duplexes fill nearly every cell of every other anti-diagonal and run out of tier 0's cells in the middle
of a step, so that tier 1 continues their state dumps."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP = {"A": "U", "C": "G", "G": "C", "U": "A"}
KNOBS = ("PRB_GAPPED_FRONT", "PRB_GAPPED_POOL")
SETTINGS = [{}, {"PRB_GAPPED_POOL": "0"}, {"PRB_GAPPED_FRONT": "0"}, {"PRB_GAPPED_FRONT": "0", "PRB_GAPPED_POOL": "0"}]
OPTS = [(x, m) for x in (1, 16, 30) for m in (1, 3, 7)]


def _rand(rng, n, gc):
    return "".join(rng.choice("GC") if rng.random() < gc else rng.choice("AU") for _ in range(n))


def _partner(rng, s, mut, indel):
    out = []
    for c in reversed(s):
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out.append(rng.choice("ACGU"))
        out.append(rng.choice("ACGU") if rng.random() < mut else COMP[c])
    return "".join(out)


def _mixed(seed):
    rng = random.Random(seed)
    qs, db = [], []
    for t in range(4):  # dense, gapped duplexes
        q = _rand(rng, rng.randint(150, 220), 0.75)
        a = rng.randint(0, len(q) // 2)
        qs.append(q)
        db.append(_rand(rng, 30, 0.5) + _partner(rng, q[a:a + rng.randint(50, 90)], 0.08, 0.04) + _rand(rng, 30, 0.5))
    for t in range(2):  # alternating G and C on both sides
        qs.append(_rand(rng, 20, 0.5) + "GC" * rng.randint(35, 55) + _rand(rng, 20, 0.5))
        db.append(_rand(rng, 20, 0.5) + "GC" * rng.randint(35, 55) + _rand(rng, 20, 0.5))
    qs += [_rand(rng, 200, 0.4) for _ in range(3)]  # hits that find little
    db += [_rand(rng, 250, 0.4) for _ in range(4)]
    order = list(range(len(db)))
    rng.shuffle(order)
    return qs, [db[i] for i in order]


@pytest.fixture(scope="module")
def setup(tmp_path_factory, oracle):
    from priblast_amd import capi
    ctx = capi.Context(0)
    qs, dbs = _mixed(6061)
    prefix = str(tmp_path_factory.mktemp("pool") / "db")
    capi.db_build(ctx, prefix, [f"d{i}" for i in range(len(dbs))], dbs, 0, 8, 70, 5)
    db = capi.Db(ctx, prefix)
    odb = oracle.Db(prefix)
    qb = capi.QBatch(ctx, qs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    yield ctx, qs, db, odb, qb
    qb.close()
    db.close()
    odb.close()
    ctx.close()


@pytest.mark.parametrize("x,m", OPTS, ids=[f"x{x}-m{m}" for x, m in OPTS])
def test_pooled_fill_matches_group_fill_and_oracle(setup, oracle, monkeypatch, x, m):
    from priblast_amd import capi
    ctx, qs, db, odb, qb = setup
    opts = capi.default_opts(output_style=1, drop_out_w_gap=x, min_helix_length=m)
    total = 0
    try:
        for page in range(db.npages):
            runs = []
            for env in SETTINGS:
                for k in KNOBS:
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                runs.append(capi.search_page(ctx, qb, db, page, opts))
            h0, bp0, c0 = runs[0]
            for env, (h1, bp1, c1) in zip(SETTINGS[1:], runs[1:]):
                assert c0 == c1, (env, page)
                assert np.array_equal(h0, h1) and np.array_equal(bp0, bp1), (env, page)
            oopts = oracle.default_opts(drop_w_gap=x, min_helix=m)
            for q, s in enumerate(qs):
                _, _, gap = odb.stages(s, page, oopts)
                mine = h0[h0["query"] == q]
                assert len(mine) == len(gap), (page, q)
                key = lambda h: (h["db_sp"], h["q_sp"], -h["db_len"], -h["q_len"], h["e_tot"])
                for a, b in zip(sorted(mine, key=key), sorted(gap, key=key)):
                    for k in ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start"):
                        assert a[k] == b[k], (page, q, k)
                    assert float(a["e_tot"]) == b["e_tot"] and float(a["e_acc"]) == b["e_acc"], (page, q)
                    assert np.array_equal(bp0[a["bp_offset"]:a["bp_offset"] + a["bp_count"]], b["bp"]), (page, q)
                total += len(mine)
    finally:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
    assert total > 0
