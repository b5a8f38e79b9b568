"""GPU tests of the evalset's kernels on hand-made lists (prb_evalset_add_keys runs the append kernel of
prb_search_page_scored / _null_hits on a caller's list; close and score are the real ones): 3 queries on the 2-page
database of 5 + 3 short targets of test_gpu_null_kernel.py.  The yardstick is tests/eval_ref.py; all five integers of
every record must be equal.  Nothing here searches: the database and the batch only give the table its shape."""
import os
import re

import numpy as np
import pytest

import eval_ref

pytestmark = pytest.mark.gpu
NQ, NSEQ = 3, (5, 3)
STATE = -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "priblast_amd", "csrc", "search_kernels.hpp")) as _f:
    CHUNK = int(re.search(r"kEvalChunk = (\d+);", _f.read()).group(1))  # the entries k_eval_qmin scans at a time


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape(ctx, tmp_path_factory):
    from priblast_amd import capi
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGU"), 40)) for _ in range(sum(NSEQ))]
    prefix = str(tmp_path_factory.mktemp("evaldb") / "edb")
    capi.db_build(ctx, prefix, [f"t{i}" for i in range(len(seqs))], seqs, page_size=5)
    db = capi.Db(ctx, prefix)
    assert db.npages == 2 and tuple(db.page_info(p)[0] for p in range(2)) == NSEQ
    qb = capi.QBatch(ctx, ["".join(rng.choice(list("ACGU"), 30)) for _ in range(NQ)], db.repeat_flag)
    yield db, qb
    qb.close()
    db.close()


def code_of(exc):
    return int(str(exc.value).split("error ")[1].split(":")[0])


def run(ctx, shape, m, real, decoy, look=None, calls=1, perm=None):
    """real / decoy = (query or owner [], energy []) -> the records of `look` (by default: of every real hit).  The lists
    are added in the order `perm` (a seed) and in `calls` pieces each, real and decoy pieces alternating."""
    from priblast_amd import capi
    db, qb = shape
    lists = []
    for ids, e in (real, decoy):
        ids, e = np.asarray(ids, np.int32), np.asarray(e, np.float64)
        if perm is not None:
            o = np.random.default_rng(perm).permutation(len(ids))
            ids, e = ids[o], e[o]
        lists.append((np.array_split(ids, calls), np.array_split(e, calls)))
    with capi.EvalSet(ctx, qb, db, m) as es:
        for k in range(calls):
            for is_decoy in (0, 1):
                es.add_keys(is_decoy, lists[is_decoy][0][k], lists[is_decoy][1][k])
        assert es.sizes() == (len(real[0]), len(decoy[0]))
        es.finish()
        lq, le = real if look is None else look
        return es.score(lq, le)


def same(got, want):
    for f in ("decoys", "null_le", "rank", "q_num", "q_den"):
        assert np.array_equal(got[f].astype(np.int64), want[f]), f
    assert not got["reserved"].any()


def lists_of(lengths, seed, decoys_per_query=(40, 300, 7), step=0.5):
    """real lists of the given lengths per query and decoy lists, energies on a grid (equal ones occur)"""
    rng = np.random.default_rng(seed)
    rq = np.concatenate([np.full(n, q) for q, n in enumerate(lengths)]).astype(np.int32)
    re_ = np.round(rng.normal(-12, 4, len(rq)) / step) * step
    dq = np.concatenate([np.full(n, q) for q, n in enumerate(decoys_per_query)]).astype(np.int32)
    de = np.round(rng.normal(-9, 4, len(dq)) / step) * step
    return (rq, re_), (dq, de)


@pytest.mark.parametrize("lengths", [(1, 63, 64), (65, CHUNK - 1, CHUNK), (CHUNK + 1, 2 * CHUNK + 3, 1)])
def test_segment_lengths_around_the_wavefront_and_the_chunk(ctx, shape, lengths):
    real, decoy = lists_of(lengths, seed=sum(lengths))
    same(run(ctx, shape, 3, real, decoy), eval_ref.score(NQ, *real, *decoy, 3))


def test_the_carry_crosses_a_chunk_boundary(ctx, shape):
    """Query 1 has 3 chunks of real hits.  Its decoys all lie between the second-highest and the highest real energy but
    for a few at the very bottom, so FDR falls to its minimum at the LAST entry of the segment - the first chunk that the
    kernel scans - while the hits looked up are the lowest ones, in the chunk it scans last: their q-value is right only
    if the carry went through both chunk boundaries."""
    n = 2 * CHUNK + 40
    re_ = -100.0 + 0.125 * np.arange(n)                 # distinct, ascending
    rq = np.full(n, 1, np.int32)
    # 3 decoys below everything (FDR 3 / (M rank): falling with the rank), none in between: the minimum is the last entry's
    de = np.array([-200.0, -201.0, -202.0])
    dq = np.full(3, 1, np.int32)
    m = 2
    want = eval_ref.score(NQ, rq, re_, dq, de, m, look_q=rq[:5], look_e=re_[:5])
    assert (want["q_num"] == 3).all() and (want["q_den"] == n).all()   # the minimiser is the highest entry
    same(run(ctx, shape, m, (rq, re_), (dq, de), look=(rq[:5], re_[:5])), want)
    # ... and with 10 more decoys just below the first chunk's lowest entry, FDR jumps there: the minimiser is the entry
    # right below that chunk (13 / n > 3 / (n - CHUNK) for these sizes), and the carry crosses one boundary
    de2 = np.append(de, np.full(10, re_[n - CHUNK] - 0.01))
    dq2 = np.full(len(de2), 1, np.int32)
    want2 = eval_ref.score(NQ, rq, re_, dq2, de2, m, look_q=rq[:5], look_e=re_[:5])
    assert (want2["q_num"] == 3).all() and (want2["q_den"] == n - CHUNK).all()
    same(run(ctx, shape, m, (rq, re_), (dq2, de2), look=(rq[:5], re_[:5])), want2)


def test_all_equal_keys_an_empty_decoy_list_and_an_empty_real_list(ctx, shape):
    # query 0: every key equal (and equal to its decoys'); query 1: no real hits, but decoys; query 2: no decoys
    rq = np.array([0] * (CHUNK + 5) + [2] * 70, np.int32)
    re_ = np.array([-9.5] * (CHUNK + 5) + list(-20 + 0.25 * np.arange(70)))
    dq = np.array([0] * 4 + [1] * 9, np.int32)
    de = np.array([-9.5] * 4 + [-30.0] * 9)
    got = run(ctx, shape, 2, (rq, re_), (dq, de))
    same(got, eval_ref.score(NQ, rq, re_, dq, de, 2))
    assert (got["null_le"][rq == 0] == 4).all() and (got["rank"][rq == 0] == CHUNK + 5).all()
    assert (got["null_le"][rq == 2] == 0).all() and (got["q_num"][rq == 2] == 0).all()
    # no decoy at all, and -0.0 beside +0.0 and a positive energy
    rq, re_ = np.array([1, 1, 1, 0], np.int32), np.array([-0.0, 0.0, 3.5, -4.0])
    same(run(ctx, shape, 5, (rq, re_), ([], [])), eval_ref.score(NQ, rq, re_, [], [], 5))


def test_a_minimum_above_one_and_equal_fractions(ctx, shape):
    real = ([0, 1, 1, 1, 1], [-10.0, -14.0, -16.0, -18.0, -20.0])
    decoy = ([0] * 5 + [1, 1], [-12.0, -11.0, -10.5, -13.0, -10.0, -19.0, -17.0])
    got = run(ctx, shape, 1, real, decoy)
    same(got, eval_ref.score(NQ, *real, *decoy, 1))
    assert (got["q_num"][0], got["q_den"][0]) == (1, 1) and got["null_le"][0] == 5   # 5 / 1 > 1 -> (M, 1)
    assert [(r["q_num"], r["q_den"]) for r in got[1:]] == [(2, 4), (2, 4), (1, 2), (0, 1)]


def test_the_order_and_the_cut_of_the_lists_do_not_matter(ctx, shape):
    real, decoy = lists_of((CHUNK + 9, 130, 64), seed=3)
    want = eval_ref.score(NQ, *real, *decoy, 4)
    base = run(ctx, shape, 4, real, decoy)
    same(base, want)
    for calls, perm in ((1, 7), (5, None), (3, 8)):
        assert run(ctx, shape, 4, real, decoy, look=real, calls=calls, perm=perm).tobytes() == base.tobytes()


def test_an_owner_out_of_range_fails_the_next_call(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    for is_decoy, ids in ((1, [0, NQ]), (0, [-1]), (1, [2 ** 31 - 1])):
        with capi.EvalSet(ctx, qb, db, 2) as es:
            es.add_keys(0, [0], [-9.0])
            es.add_keys(is_decoy, ids, [-9.0] * len(ids))   # (the kernel raises the flag and writes nothing)
            for call in (lambda: es.add_keys(0, [0], [-8.0]), es.finish):
                with pytest.raises(capi.PrbError) as e:
                    call()
                assert code_of(e) == STATE


def test_a_key_that_is_not_in_the_table_fails_the_score(ctx, shape):
    from priblast_amd import capi
    db, qb = shape
    for q, e in ((0, -9.25), (1, -9.0), (NQ, -9.0)):
        with capi.EvalSet(ctx, qb, db, 2) as es:
            es.add_keys(0, [0, 0], [-9.0, -9.5])
            es.add_keys(1, [0], [-9.0])
            with pytest.raises(capi.PrbError) as ex:   # (not closed yet)
                es.score([0], [-9.0])
            assert code_of(ex) == STATE
            es.finish()
            assert es.score([0], [-9.0])["rank"][0] == 2
            with pytest.raises(capi.PrbError) as ex:
                es.score([0, q], [-9.0, e])
            assert code_of(ex) == STATE
            with pytest.raises(capi.PrbError) as ex:   # (closed: nothing is added)
                es.add_keys(0, [0], [-1.0])
            assert code_of(ex) == STATE
