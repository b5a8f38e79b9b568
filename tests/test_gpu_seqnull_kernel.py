"""GPU tests of the null table's retiring pass and of the live mask made on the device, through the C ABI on hand-made
records (prb_nullset_observe, prb_nullset_add_pairs, prb_nullset_retire, prb_pairmask_create_live).  The databases are cut
from a few golden sequences so that the target counts cover the edges of the mask's 32-bit words and of a wavefront's 64
slots: 1, 31, 32, 33, 63, 64, 65 and 129 targets on one page, and 5 + 3 on two.  With 3 queries a wavefront of the retiring
pass lies across the queries' rows at every one of them (at 33 targets: 33 + 31 slots).  The yardstick is
tests/seqnull_ref.py's fold of the same lists.  Nothing here searches: the databases and the batches only give the tables
and the masks their shape."""
import os

import numpy as np
import pytest

import refdump
import seqnull_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NQ, N, H, R = 3, 6, 2, 2
STATE, ARG = -5, -1
SHAPES = {"t1": (1,), "t31": (31,), "t32": (32,), "t33": (33,), "t63": (63,), "t64": (64,), "t65": (65,), "t129": (129,), "p5_3": (5, 3)}
ROWS = [2, 0, 0, 1, 2, 0, 2]  # the owners of a decoy batch's rows: not grouped, not ascending


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shapes(ctx, tmp_path_factory):
    """name -> (db, the real batch of 3 queries, a decoy batch of len(ROWS) queries), built when first asked for"""
    from priblast_amd import capi
    _, gold = refdump.read_fasta(os.path.join(HERE, "golden", "mix_db.fa"))
    made = {}

    def get(name):
        if name not in made:
            nseq = SHAPES[name]
            seqs = [gold[i % len(gold)][(12 * (i // len(gold))) % (len(gold[i % len(gold)]) - 40):][:40] for i in range(sum(nseq))]
            prefix = str(tmp_path_factory.mktemp("seqnull_" + name) / "db")
            capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(seqs))], seqs, page_size=nseq[0])
            db = capi.Db(ctx, prefix)
            assert tuple(db.page_info(p)[0] for p in range(db.npages)) == nseq
            made[name] = (db, capi.QBatch(ctx, [gold[q][:30] for q in range(NQ)], db.repeat_flag),
                          capi.QBatch(ctx, [gold[k][:25] for k in range(len(ROWS))], db.repeat_flag))
        return made[name]

    yield get
    for db, qb, dqb in made.values():
        dqb.close()
        qb.close()
        db.close()


def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records with every other field filled in recognisably"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + i % 3, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def scenario(nseq, seed):
    """-> (observed [NQ, T] bool, hit [N, NQ, T] in {0: none, 1: weaker than the pair, 2: reaches it}): about 0.7 of the
    pairs are observed - every query's first and last target among them -, and a decoy hits a target - observed or not -
    half of the time, reaching the pair's energy half of those"""
    T = sum(nseq)
    rng = np.random.default_rng(seed)
    observed = rng.random((NQ, T)) < 0.7
    observed[:, 0] = observed[:, T - 1] = True
    hit = rng.integers(0, 4, (N, NQ, T)).clip(1, 3) - 1
    return observed, hit


def page_of(nseq, t):
    p = 0
    while t >= nseq[p]:
        t -= nseq[p]
        p += 1
    return p, t


def lists(nseq, observed, hit):
    """the scenario as seqnull_ref.fold takes it: (real, decoys)"""
    T = sum(nseq)
    real = {p: [] for p in range(len(nseq))}
    for q in range(NQ):
        for t in range(T):
            if observed[q, t]:
                p, i = page_of(nseq, t)
                real[p].append((q, i, -10.0 - q))
    decoys = []
    for q in range(NQ):
        for d in range(N):
            pages = {p: [] for p in range(len(nseq))}
            for t in range(T):
                if hit[d, q, t]:
                    p, i = page_of(nseq, t)
                    pages[p].append((0, i, (-10.0 - q) + (1.0 if hit[d, q, t] == 1 else -0.5 * d)))
            decoys.append((q, d, {p: pairs(r) for p, r in pages.items()}))
    return {p: pairs(r) for p, r in real.items()}, decoys


def add_round(ns, nseq, decoys, lo, hi, queries=range(NQ)):
    """the decoys [lo, hi) of `queries` into the table, one call per page"""
    part = [(q, d, pages) for q, d, pages in decoys if lo <= d < hi and q in queries]
    for p in range(len(nseq)):
        recs = []
        for k, (_, _, pages) in enumerate(part):
            r = pages[p].copy()
            r["query"] = k
            recs.append(r)
        ns.add_pairs(p, [q for q, _, _ in part], [d for _, d, _ in part], np.concatenate(recs) if recs else pairs([]))


def live_words(live):
    """live [NQ, T] bool -> the rows of a mask of ROWS: uint32 [len(ROWS), (T + 31) // 32], the bits beyond T zero"""
    T = live.shape[1]
    out = np.zeros((len(ROWS), (T + 31) // 32), np.uint32)
    for k, q in enumerate(ROWS):
        for t in np.flatnonzero(live[q]):
            out[k, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return out


def check_mask(ctx, ns, dqb, live):
    from priblast_amd import capi
    with capi.PairMask.live(ctx, ns, dqb, ROWS) as pm:
        got, want = pm.words(len(ROWS)), live_words(live)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)
        assert pm.count == int(sum(live[q].sum() for q in ROWS))
        with pytest.raises(capi.PrbError) as e:  # born used
            pm.allow([0], [0], [0])
        assert code_of(e) == STATE


@pytest.mark.parametrize("name", list(SHAPES))
def test_retire_and_live_mask_at_every_edge(ctx, shapes, name):
    from priblast_amd import capi
    db, qb, dqb = shapes(name)
    nseq = SHAPES[name]
    observed, hit = scenario(nseq, 100 + sum(nseq))
    real, decoys = lists(nseq, observed, hit)
    le = np.cumsum(hit == 2, axis=0)  # [b - 1, q, t] = NullLE(b)
    with capi.NullSet(ctx, qb, db, N) as ns:
        for p in range(len(nseq)):
            ns.observe(p, real[p])
        check_mask(ctx, ns, dqb, observed)  # nothing has retired: the live pairs are the observed ones
        for b in seqnull_ref.boundaries(N, R):
            add_round(ns, nseq, decoys, b - R, b)  # every query's, so records arrive for retired pairs too
            live = observed & (le[b - 1] < H)
            left = ns.retire(H, b)
            assert left.tolist() == live.sum(axis=1).tolist(), (b, left)
            check_mask(ctx, ns, dqb, live)
        got = ns.finish()
    want = seqnull_ref.fold(real, decoys, N, H, R)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert len(got) == observed.sum() and set(got["decoys"].tolist()) <= {2, 4, 6}
    # a retired pair kept its first `seen` and its counters over the later records and the later retire calls
    for r in got:
        p0 = sum(nseq[:int(r["page"])])
        first = int(np.argmax(le[:, int(r["query"]), p0 + int(r["db_id"])] >= H)) + 1 if r["null_le"] >= H else N
        assert int(r["decoys"]) == min(N, -(-first // R) * R) and r["null_le"] == le[int(r["decoys"]) - 1, int(r["query"]), p0 + int(r["db_id"])]


def test_some_shape_shows_every_case():
    """the scenarios above retire pairs at the first boundary, at a later one and not at all, and a retired pair's
    columns differ from those of all N decoys"""
    nseq = SHAPES["t33"]
    observed, hit = scenario(nseq, 100 + sum(nseq))
    assert all(seqnull_ref.shows_every_case(*lists(nseq, observed, hit), N, H, R).values())


def test_a_query_without_live_pairs_needs_no_further_decoys(ctx, shapes):
    """query 1's pairs all retire at the first boundary: the later rounds leave it out, and the table finishes"""
    from priblast_amd import capi
    db, qb, dqb = shapes("t33")
    nseq = SHAPES["t33"]
    observed, hit = scenario(nseq, 7)
    hit[:2, 1, :] = 2
    observed[2, :] = False  # and query 2 has no pair at all
    real, decoys = lists(nseq, observed, hit)
    with capi.NullSet(ctx, qb, db, N) as ns:
        ns.observe(0, real[0])
        add_round(ns, nseq, decoys, 0, 2)
        left = ns.retire(H, 2)
        assert left[1] == 0 and left[2] == 0 and left[0] > 0
        with pytest.raises(capi.PrbError) as e:  # query 0 still has live pairs
            ns.finish()
        assert code_of(e) == STATE and "live pairs" in str(e.value)
        add_round(ns, nseq, decoys, 2, 4, queries=[0])
        ns.retire(H, 4)
        add_round(ns, nseq, decoys, 4, 6, queries=[0])
        got = ns.finish()
    assert got.tobytes() == seqnull_ref.fold(real, decoys, N, H, R).tobytes()
    assert (got["decoys"][got["query"] == 1] == 2).all() and (got["query"] != 2).all()


def test_new_guards_refuse_and_leave_the_table_as_it_was(ctx, shapes):
    from priblast_amd import capi
    db, qb, dqb = shapes("p5_3")
    nseq = SHAPES["p5_3"]
    observed, hit = scenario(nseq, 3)
    real, decoys = lists(nseq, observed, hit)

    def refused(code, word, fn, *args):
        with pytest.raises(capi.PrbError) as e:
            fn(*args)
        assert code_of(e) == code and word in str(e.value), str(e.value)

    with capi.NullSet(ctx, qb, db, N) as ns:
        ns.observe(0, real[0])
        refused(STATE, "not observed", ns.retire, H, 2)          # a page is not observed yet
        ns.observe(1, real[1])
        refused(STATE, "is not merged", ns.retire, H, 2)         # no decoy is merged
        add_round(ns, nseq, decoys, 0, 2, queries=[0, 1])
        refused(STATE, "of query 2 is not merged", ns.retire, H, 2)  # one query's decoys are missing
        add_round(ns, nseq, decoys, 0, 2, queries=[2])
        refused(ARG, "min_le", ns.retire, 0, 2)
        refused(ARG, "upto", ns.retire, H, 0)
        refused(ARG, "upto", ns.retire, H, N + 1)
        refused(STATE, "is not merged", ns.retire, H, 4)         # decoys 2 and 3 are not merged
        refused(ARG, "owner", capi.PairMask.live, ctx, ns, dqb, [0, 1, NQ, 0, 0, 0, 0])
        refused(ARG, "owner", capi.PairMask.live, ctx, ns, dqb, [0, 1, -1, 0, 0, 0, 0])
        refused(ARG, "queries", capi.PairMask.live, ctx, ns, dqb, [0, 1])
        check_mask(ctx, ns, dqb, observed)                       # none of them retired anything
        ns.retire(H, 2)
        refused(ARG, "upto", ns.retire, H, 2)                    # not above the call before
        refused(ARG, "upto", ns.retire, H, 1)
        for b in (4, 6):
            add_round(ns, nseq, decoys, b - R, b)
            ns.retire(H, b)
        got = ns.finish()
        refused(STATE, "finished", ns.retire, H, 6)
        refused(STATE, "finished", capi.PairMask.live, ctx, ns, dqb, ROWS)
    assert got.tobytes() == seqnull_ref.fold(real, decoys, N, H, R).tobytes()  # none of the refused calls left a trace


def test_a_table_that_never_retires_is_the_plain_table(ctx, shapes):
    """retiring at N only, with min_le = N: no pair can retire before it has seen every decoy"""
    import null_ref
    from priblast_amd import capi
    db, qb, dqb = shapes("t65")
    nseq = SHAPES["t65"]
    observed, hit = scenario(nseq, 5)
    real, decoys = lists(nseq, observed, hit)
    with capi.NullSet(ctx, qb, db, N) as ns:
        ns.observe(0, real[0])
        add_round(ns, nseq, decoys, 0, N)
        ns.retire(N, N)
        got = ns.finish()
    assert got.tobytes() == null_ref.fold(real, decoys, N).tobytes() and (got["decoys"] == N).all()
