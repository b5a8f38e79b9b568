"""GPU tests of the q-value ranking of the null table (prb_nullset_finish_fdr), through the C ABI on hand-made records, as
test_gpu_seqnull_kernel.py builds its tables (prb_nullset_observe, prb_nullset_add_pairs, prb_nullset_retire).  Nothing
here searches.  3 queries; the target counts cover a wavefront's 64 lanes (1, 63, 64, 65, 129), two pages (5 + 3) and the
chunk of the step-up pass, which the library exports as prb_fdr_chunk() and this file assumes to be CHUNK = 256: one more
than a chunk (257) and two chunks plus one (513).  Query 0 has no observed pair, query 1 exactly one, query 2 every target
but one (so its q-values of p = 1 exceed 1 and are capped).
The yardstick is tests/fdr_ref.py on the (query, null_le, decoys) of the records alone."""
import os
from fractions import Fraction

import numpy as np
import pytest

import fdr_ref
import refdump

HERE = os.path.dirname(os.path.abspath(__file__))
NQ, N, H = 3, 7, 1
BOUNDS = (1, 3, 7)  # prb_nullset_retire's `upto`s: denominators 2, 4 and 8, so 1/2 = 2/4 = 4/8 and 1 = 2/2 = 4/4 = 8/8 can tie
CHUNK = 256
STATE, ARG = -5, -1
# (query 2 leaves one target unobserved, so c258 and c514 are the shapes whose segment is one more than a chunk / than two)
SHAPES = {"t1": (1,), "t63": (63,), "t64": (64,), "t65": (65,), "t129": (129,), "p5_3": (5, 3), "c257": (CHUNK + 1,), "c258": (CHUNK + 2,),
          "c513": (2 * CHUNK + 1,), "c514": (2 * CHUNK + 2,)}


def page_of(nseq, t):
    p = 0
    while t >= nseq[p]:
        t -= nseq[p]
        p += 1
    return p, t


def scenario(nseq, seed=0):
    """-> (observed [NQ, T] bool, reach [N, NQ, T] bool: decoy d reaches the pair's energy).  Query 2's targets fall into
    four kinds: strong (no decoy reaches them), tied (only decoy 1 or 2 does: they retire at 3 with 2/4), half (decoys 3, 4
    and 5: never retired before 7, 4/8) and weak (decoy 0: retired at 1 with 2/2).  Beyond a chunk the strong ones are few, so
    that their minimiser is the run of 1/2 - further up in the sorted segment."""
    T = sum(nseq)
    rng = np.random.default_rng(1000 + T + seed)
    observed = np.zeros((NQ, T), bool)
    observed[1, T // 2] = True
    observed[2, :] = True
    if T >= 8:
        observed[2, 4] = False
    reach = np.zeros((N, NQ, T), bool)
    kind = rng.integers(0, 4, T) if T <= CHUNK else rng.choice(4, T, p=[0.1, 0.4, 0.4, 0.1])
    kind[T - 1] = 0  # a strong pair exists whatever the draw
    if T >= 8:
        kind[:8] = [0, 1, 2, 3, 1, 2, 0, 0]
    reach[1, 2, kind == 1] = True
    for d in (3, 4, 5):
        reach[d, 2, kind == 2] = True
    reach[0, 2, kind == 3] = True
    reach[2, 1, T // 2] = True
    return observed, reach


def expected(nseq, observed, reach):
    """the (query, null_le, decoys) of every record in the finish's order: by query, then target"""
    out = []
    for q in range(NQ):
        for t in range(sum(nseq)):
            if observed[q, t]:
                seen = next((b for b in BOUNDS if reach[:b, q, t].sum() >= H), N)
                out.append((q, int(reach[:seen, q, t].sum()), seen))
    return out


def pairs(rows):
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + i % 3, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


def fill(ns, nseq, observed, reach, rng=None):
    """the scenario into the table: the pages observed, then round by round the decoys of every query - one add_pairs call
    per page, the pages and the decoys of a round in the order of rng (None: ascending) - and the retire at the round's end"""
    T = sum(nseq)
    pages = list(range(len(nseq)))
    if rng is not None:
        rng.shuffle(pages)
    for p in pages:
        ns.observe(p, pairs([(q, page_of(nseq, t)[1], -10.0) for q in range(NQ) for t in range(T) if observed[q, t] and page_of(nseq, t)[0] == p]))
    lo = 0
    for b in BOUNDS:
        part = [(q, d) for q in range(NQ) for d in range(lo, b)]
        if rng is not None:
            rng.shuffle(part)
            rng.shuffle(pages)
        for p in pages:
            rows = [(k, page_of(nseq, t)[1], -11.0) for k, (q, d) in enumerate(part) for t in range(T) if reach[d, q, t] and page_of(nseq, t)[0] == p]
            ns.add_pairs(p, [q for q, _ in part], [d for _, d in part], pairs(rows))
        ns.retire(H, b)
        lo = b


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shapes(ctx, tmp_path_factory):
    from priblast_amd import capi
    _, gold = refdump.read_fasta(os.path.join(HERE, "golden", "mix_db.fa"))
    made = {}

    def get(name):
        if name not in made:
            nseq = SHAPES[name]
            seqs = [gold[i % len(gold)][(7 * (i // len(gold))) % (len(gold[i % len(gold)]) - 40):][:40] for i in range(sum(nseq))]
            prefix = str(tmp_path_factory.mktemp("fdr_" + name) / "db")
            capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(seqs))], seqs, page_size=nseq[0])
            db = capi.Db(ctx, prefix)
            assert tuple(db.page_info(p)[0] for p in range(db.npages)) == nseq
            made[name] = (db, capi.QBatch(ctx, [gold[q][:30] for q in range(NQ)], db.repeat_flag))
        return made[name]

    yield get
    for db, qb in made.values():
        qb.close()
        db.close()


def figures(got):
    return [(int(f["tests"]), int(f["rank"]), int(f["q_num"]), int(f["q_den"]), int(f["q_rank"])) for f in got]


def test_the_scenarios_show_every_case():
    """on the reference's figures alone (no GPU): the ties, the cap, the share below 1 and a minimiser beyond the chunk"""
    for name, nseq in SHAPES.items():
        T = sum(nseq)
        observed, reach = scenario(nseq)
        want = expected(nseq, observed, reach)
        assert sum(1 for w in want if w[0] == 0) == 0 and sum(1 for w in want if w[0] == 1) == 1
        figs = fdr_ref.fdr(want, {q: T for q in range(NQ)})
        mine = [(w, f) for w, f in zip(want, figs) if w[0] == 2]
        assert len(mine) == (T - 1 if T >= 8 else T)
        if T >= 8:
            dens = {(le + 1, d + 1) for (q, le, d), _ in mine}
            assert {(1, 8), (2, 4), (4, 8), (2, 2)} <= dens  # 2/4 against 4/8: equal p-values with different denominators
            below = sum(1 for _, f in mine if f[2:] != (0, 0, 0) and fdr_ref.q_value(f[0], *f[2:]) < 1)
            assert 3 * below >= len(mine) and any(f[2:] == (0, 0, 0) for _, f in mine), (name, below, T)
            # the tie decides a triple: a pair of p = 1/2 whose minimiser is one of the run with the lower denominator
            assert any(f[2:4] == (2, 4) for (q, le, d), f in mine if (le + 1, d + 1) == (4, 8))
        if len(mine) > CHUNK:
            # Sorted by p-value the strong pairs (1/8) lie first, the run of 1/2 behind them.  The step-up pass cuts a segment
            # into chunks from its END: the strong pair at place 0 is served by the run of 1/2, whose pairs of 2/4 lie in chunks
            # that the pass takes earlier - the minimum reaches the pair through the carry.
            n = len(mine)
            order = sorted(range(n), key=lambda i: Fraction(mine[i][0][1] + 1, mine[i][0][2] + 1))
            chunk_of = lambda k: (n - 1 - k) // CHUNK
            minimisers = [k for k, i in enumerate(order) if (mine[i][0][1] + 1, mine[i][0][2] + 1) == (2, 4)]
            assert mine[order[0]][0][1:] == (0, N) and mine[order[0]][1][2:4] == (2, 4), name
            assert any(chunk_of(k) < chunk_of(0) for k in minimisers), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_figures_equal_the_reference_at_every_edge(ctx, shapes, name):
    from priblast_amd import capi
    assert capi.lib().prb_fdr_chunk() == CHUNK
    db, qb = shapes(name)
    nseq = SHAPES[name]
    T = sum(nseq)
    observed, reach = scenario(nseq)
    want = expected(nseq, observed, reach)
    with capi.NullSet(ctx, qb, db, N) as twin:
        fill(twin, nseq, observed, reach)
        plain = twin.finish()
        assert capi.lib().prb_nullset_fdr(twin.h) is None  # (a plain finish has no figures)
        twin.finish_fdr()  # ... and a later finish_fdr does nothing
        assert capi.lib().prb_nullset_fdr(twin.h) is None and capi.lib().prb_nullset_size(twin.h) == len(plain)
    assert [(int(r["query"]), int(r["null_le"]), int(r["decoys"])) for r in plain] == want
    count = [sum(1 for w in want if w[0] == q) for q in range(NQ)]
    first = None
    for tests in (None, [max(1, c) for c in count], [2 ** 31 - 1] * NQ):
        for order in (None, 1, 2):
            with capi.NullSet(ctx, qb, db, N) as ns:
                fill(ns, nseq, observed, reach, None if order is None else np.random.default_rng(order))
                recs, got = ns.finish_fdr(tests)
            assert recs.tobytes() == plain.tobytes()  # byte for byte the records of prb_nullset_finish
            ref = fdr_ref.fdr(want, {q: T for q in range(NQ)} if tests is None else tests)
            assert figures(got) == ref, (name, tests, order)
            if order is None:
                first = got.tobytes()
            assert got.tobytes() == first  # the same bytes whatever the order of the observe / add_pairs calls
            if tests is not None:
                break  # (the order of the calls is varied under the first `tests` only)


@pytest.mark.gpu
def test_refusals_leave_the_table_as_documented(ctx, shapes):
    from priblast_amd import capi
    db, qb = shapes("p5_3")
    nseq = SHAPES["p5_3"]
    observed, reach = scenario(nseq)
    want = expected(nseq, observed, reach)

    def refused(code, word, fn, *args):
        with pytest.raises(capi.PrbError) as e:
            fn(*args)
        assert code_of(e) == code and word in str(e.value), str(e.value)

    with capi.NullSet(ctx, qb, db, N) as ns:
        for p in range(len(nseq)):
            ns.observe(p, pairs([(q, page_of(nseq, t)[1], -10.0) for q in range(NQ) for t in range(8) if observed[q, t] and page_of(nseq, t)[0] == p]))
        refused(STATE, "searches are merged", ns.finish_fdr)               # the refusals of prb_nullset_finish come first
        refused(STATE, "searches are merged", ns.finish_fdr, [0, 0, 0])
    with capi.NullSet(ctx, qb, db, N) as ns:
        fill(ns, nseq, observed, reach)
        refused(ARG, "tests[0] = 0", ns.finish_fdr, [0, 1, 8])             # below 1 (on the host, before anything is enqueued)
        refused(ARG, "tests[1] = -3", ns.finish_fdr, [1, -3, 8])
        refused(ARG, "tests[2] = 2147483648", ns.finish_fdr, [1, 1, 2 ** 31])
        refused(ARG, "is below the 7 observed pairs of query 2", ns.finish_fdr, [1, 1, 6])  # counted on the device, checked before the ranking
        recs, got = ns.finish_fdr([1, 1, 7])                               # every refusal left the table usable
        assert figures(got) == fdr_ref.fdr(want, [1, 1, 7]) and len(recs) == 8
        again, got2 = ns.finish_fdr([5, 5, 50])                            # a second finish does nothing
        assert again.tobytes() == recs.tobytes() and got2.tobytes() == got.tobytes()
        assert ns.finish().tobytes() == recs.tobytes()
        refused(STATE, "finished", ns.retire, H, N)
    with capi.NullSet(ctx, qb, db, N) as twin:
        fill(twin, nseq, observed, reach)
        assert twin.finish().tobytes() == recs.tobytes()
    # the line writer of the C ABI on these records: the lines of prb_write_null_lines with the three columns behind
    names, qlen = ["qa", "qb", "qc"], [30, 30, 30]
    import tempfile
    texts = []
    for write, args in ((capi.write_null_lines, (recs,)), (capi.write_null_fdr_lines, (recs, got))):
        with tempfile.TemporaryFile("w+") as f:
            lines, _ = write(db, names, qlen, *args, fd=f.fileno())
            f.seek(0)
            texts.append(f.read().splitlines())
            assert lines == len(recs)
    for a, b, fig in zip(texts[0], texts[1], figures(got)):
        assert b == a + "," + fdr_ref.columns(fig)
    bad = got.copy()
    bad["q_den"][0] = 0 if bad["q_den"][0] else 1  # neither (0, 0, 0) nor three positive numbers
    refused(ARG, "inconsistent", capi.write_null_fdr_lines, db, names, qlen, recs, bad)


@pytest.mark.gpu
def test_a_p_value_above_one_raises_bad_and_leaves_the_table_unusable(ctx, shapes):
    """All N decoys are merged - every one of them reaching both pairs - before prb_nullset_retire(1, 1) retires the pairs
    with decoys = 1: null_le = 7 exceeds the decoys seen, (7 + 1) / (1 + 1) is no p-value.  The key pass raises the table's
    `bad` flag: PRB_ERR_STATE, nothing is written, and every later call on the table is refused.  A plain finish of a twin
    table takes the same records (it ranks nothing), so the refusal is the new entry's own."""
    from priblast_amd import capi
    db, qb = shapes("p5_3")
    nseq = SHAPES["p5_3"]
    real = {0: pairs([(2, 1, -10.0), (1, 3, -10.0)]), 1: pairs([])}
    part = [(q, d) for q in range(NQ) for d in range(N)]
    hits = pairs([(k, t, -11.0) for k, (q, d) in enumerate(part) for qq, t in ((2, 1), (1, 3)) if q == qq])

    def fill_beyond(ns):
        for p in range(len(nseq)):
            ns.observe(p, real[p])
        ns.add_pairs(0, [q for q, _ in part], [d for _, d in part], hits)
        ns.add_pairs(1, [q for q, _ in part], [d for _, d in part], pairs([]))
        assert ns.retire(1, 1).tolist() == [0, 0, 0]

    def refused(word, fn, *args):
        with pytest.raises(capi.PrbError) as e:
            fn(*args)
        assert code_of(e) == STATE and word in str(e.value), str(e.value)

    with capi.NullSet(ctx, qb, db, N) as twin:
        fill_beyond(twin)
        plain = twin.finish()
        assert [(int(r["query"]), int(r["null_le"]), int(r["decoys"])) for r in plain] == [(1, N, 1), (2, N, 1)]
    with capi.NullSet(ctx, qb, db, N) as ns:
        fill_beyond(ns)
        refused("null_le exceeds the decoys", ns.finish_fdr)
        assert capi.lib().prb_nullset_size(ns.h) == 0 and capi.lib().prb_nullset_fdr(ns.h) is None  # nothing was written
        refused("outside it", ns.finish_fdr)   # unusable from here on: every entry refuses the table
        refused("outside it", ns.finish_fdr, [1, 1, 1])
        refused("outside it", ns.finish)
        refused("outside it", ns.retire, 1, 2)
        assert capi.lib().prb_nullset_size(ns.h) == 0 and capi.lib().prb_nullset_fdr(ns.h) is None
