"""The candidate scan of the LDS tiers of the gapped extension on inputs that make it work hard: GC-rich and
low-complexity sequences, whose hits fill many cells per anti-diagonal and keep long windows of live candidates, at
drop-out lengths (-x) of 1, 16 and 30.  The final hits and their base pairs must be the same with the default cascade,
with every hit going through tier 0 (PRB_GAPPED_FRONT=0), with one anti-diagonal per tier-0 step (PRB_GAPPED_PAIR=0) and
as the oracle has them.  One case is made of alternating G and C only: its extensions fill nearly every cell of every
other anti-diagonal and run out of tier 0's cells in the middle of one, so that tier 1 continues the state dumps."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP = {"A": "U", "C": "G", "G": "C", "U": "A"}


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _rand(rng, n, gc):
    return "".join(rng.choice("GC") if rng.random() < gc else rng.choice("AU") for _ in range(n))


def _partner(rng, s, mut, indel):
    """the reverse complement of s with point changes, insertions and deletions: interactions with gaps"""
    out = []
    for c in reversed(s):
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out.append(rng.choice("ACGU"))
        out.append(rng.choice("ACGU") if rng.random() < mut else COMP[c])
    return "".join(out)


def _gc_rich(seed):
    rng = random.Random(seed)
    qs = [_rand(rng, rng.randint(160, 260), 0.75) for _ in range(6)]
    db = []
    for q in qs:
        a = rng.randint(0, len(q) // 2)
        db.append(_rand(rng, 40, 0.6) + _partner(rng, q[a:a + rng.randint(60, 110)], 0.08, 0.04) + _rand(rng, 40, 0.6))
    db += [_rand(rng, 300, 0.7) for _ in range(3)]
    return qs, db


def _low_complexity(seed):
    rng = random.Random(seed)
    units = ["GGC", "GCC", "GGGCCC", "GCGCAU", "GGCGCC", "CCGG", "GGAUCC"]
    qs, db = [], []
    for t in range(6):
        u = units[t % len(units)]
        q = _rand(rng, 30, 0.5) + u * (90 // len(u)) + _rand(rng, 30, 0.5)
        qs.append("".join(c if rng.random() > 0.03 else rng.choice("ACGU") for c in q))
        db.append(_rand(rng, 30, 0.5) + _partner(rng, q[20:130], 0.05, 0.03) + _rand(rng, 30, 0.5))
    return qs, db


def _alternating_gc(seed):
    rng = random.Random(seed)
    qs = [_rand(rng, 25, 0.5) + "GC" * rng.randint(40, 60) + _rand(rng, 25, 0.5) for _ in range(3)]
    db = [_rand(rng, 25, 0.5) + "GC" * rng.randint(40, 60) + _rand(rng, 25, 0.5) for _ in range(3)]
    return qs, db


CASES = [("gc_rich", _gc_rich, 1), ("gc_rich", _gc_rich, 16), ("gc_rich", _gc_rich, 30),
         ("low_complexity", _low_complexity, 1), ("low_complexity", _low_complexity, 16), ("low_complexity", _low_complexity, 30),
         ("alternating_gc", _alternating_gc, 16), ("alternating_gc", _alternating_gc, 30)]
KNOBS = ("PRB_GAPPED_FRONT", "PRB_GAPPED_PAIR")


@pytest.mark.parametrize("name,make,x", CASES, ids=[f"{n}-x{x}" for n, _, x in CASES])
def test_dense_extensions_match_across_paths_and_oracle(ctx, oracle, tmp_path, monkeypatch, name, make, x):
    from priblast_amd import capi
    qs, dbs = make(1000 + x)
    prefix = str(tmp_path / "db")
    capi.db_build(ctx, prefix, [f"d{i}" for i in range(len(dbs))], dbs, 0, 8, 70, 5)
    db = capi.Db(ctx, prefix)
    odb = oracle.Db(prefix)
    qb = capi.QBatch(ctx, qs, db.repeat_flag)
    qb.accessibility(db.W, db.delta)
    opts = capi.default_opts(output_style=1, drop_out_w_gap=x)
    try:
        total = 0
        for page in range(db.npages):
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            h0, bp0, c0 = capi.search_page(ctx, qb, db, page, opts)
            for knob in KNOBS:
                monkeypatch.setenv(knob, "0")
                h1, bp1, c1 = capi.search_page(ctx, qb, db, page, opts)
                monkeypatch.delenv(knob)
                assert c0 == c1, (knob, page)
                assert np.array_equal(h0, h1) and np.array_equal(bp0, bp1), (knob, page)
            oopts = oracle.default_opts(drop_w_gap=x)
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
        assert total > 0
    finally:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        qb.close()
        db.close()
        odb.close()
