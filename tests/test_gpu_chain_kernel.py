"""GPU tests of the chain selection (launch_chain_select) on hand-made lists of final hits, through prb_chain_sites: the
dynamic programme restated in chain_ref.chains is the yardstick.  The random lists run with the build's LDS capacity and
with PRB_CHAIN_LDS_HITS forced small, which sends the runs of more than that many hits to the workgroup kernel with their
scores and predecessors in HBM (1: every run of two hits or more)."""
import numpy as np
import pytest

import distinct_ref
from chain_ref import chain_of_each_run, keep_mask
from distinct_ref import runs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def make(rects, energies, query=0, db_id=0):
    """one run: rects = [(q_sp, q_len, db_sp, db_len)]"""
    from priblast_amd import capi
    h = np.zeros(len(rects), capi.HIT_DTYPE)
    r = np.asarray(rects, np.int32).reshape(-1, 4)
    h["q_sp"], h["q_len"], h["db_sp"], h["db_len"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    h["e_tot"] = energies
    h["query"], h["db_id"] = query, db_id
    return h


def random_run(rng, n, query=0, db_id=0):
    """n rectangles of 4 .. 12 positions on a grid that grows slowly with n (so that chains of many hits arise and most
    hits have several predecessors), sorted by db_sp as the search's list is; energies from a coarse grid (many equal
    scores), one in eight of them zero or positive"""
    span = 60 + n // 2
    db_sp = np.sort(rng.integers(0, span, n))
    rects = np.stack([rng.integers(0, span, n), rng.integers(4, 13, n), db_sp, rng.integers(4, 13, n)], axis=1)
    e = -0.5 * rng.integers(1, 12, n)
    odd = rng.integers(0, 8, n) == 0
    e[odd] = rng.choice([0.0, -0.0, 0.5, 3.0], int(odd.sum()))
    return make(rects, e, query, db_id)


def expected_edges():
    """(list, keep) pairs that spell the rule out"""
    A, B = (0, 10, 0, 10), (20, 10, 20, 10)  # A precedes B
    return {
        "precede": (make([A, B], [-5.0, -4.0]), [1, 1]),
        "intersect": (make([A, (5, 10, 5, 10)], [-5.0, -4.0]), [1, 0]),
        "intersect_second_better": (make([A, (5, 10, 5, 10)], [-4.0, -5.0]), [0, 1]),
        "cross": (make([(50, 10, 0, 10), (0, 10, 20, 10)], [-5.0, -4.0]), [1, 0]),  # query up, target down
        "cross_second_better": (make([(50, 10, 0, 10), (0, 10, 20, 10)], [-4.0, -5.0]), [0, 1]),
        "touch_query": (make([A, (9, 10, 20, 10)], [-5.0, -4.0]), [1, 0]),   # q end == the next q_sp: a shared row
        "touch_target": (make([A, (20, 10, 9, 10)], [-5.0, -4.0]), [1, 0]),  # db end == the next db_sp: a shared column
        "adjacent": (make([A, (10, 10, 10, 10)], [-5.0, -4.0]), [1, 1]),     # end + 1 == start: chained
        # the lowest-energy single hit (the middle one) meets both others, which precede each other and together are lower
        "greedy_is_not_optimal": (make([A, (5, 30, 5, 30), B], [-6.0, -10.0, -6.0]), [1, 0, 1]),
        "single_beats_two": (make([A, (5, 30, 5, 30), B], [-4.0, -10.0, -4.0]), [0, 1, 0]),
        # equal S through two predecessors (they share their query rows: no chain of the two): the lowest place
        "tie_predecessor": (make([(0, 5, 0, 5), (0, 5, 6, 5), (10, 5, 20, 5)], [-3.0, -3.0, -2.0]), [1, 0, 1]),
        "tie_end": (make([A, (5, 10, 5, 10)], [-3.0, -3.0]), [1, 0]),
        "tie_end_of_chains": (make([A, (0, 10, 12, 10), B, (20, 10, 32, 10)], [-3.0, -3.0, -1.0, -1.0]), [1, 0, 1, 0]),
        # zero and positive energies: never chained onto, never a gain
        "positive_alone": (make([A], [2.0]), [1]),
        "positive_first": (make([A, B], [2.0, -3.0]), [0, 1]),
        "positive_second": (make([A, B], [-3.0, 2.0]), [1, 0]),
        "positives": (make([A, B], [2.0, 1.0]), [0, 1]),
        "minus_zero_first": (make([A, B], [-0.0, -3.0]), [0, 1]),
        "zero_second": (make([A, B], [-3.0, 0.0]), [1, 0]),  # S equal: the lowest place ends the chain
        "minus_zero_second": (make([A, B], [-3.0, -0.0]), [1, 0]),
        "zeros": (make([A, B], [0.0, -0.0]), [1, 0]),
        "zeros_swapped": (make([A, B], [-0.0, 0.0]), [1, 0]),
        "pairs_apart": (np.concatenate([make([A], [-9.0], 0, 0), make([B], [-8.0], 0, 1), make([B], [-8.0], 1, 1)]), [1, 1, 1]),
    }


def boundary_cases():
    rng = np.random.default_rng(11)
    out = {}
    for n in (64, 65, 129):
        out[f"run{n}"] = random_run(rng, n)
    singles = lambda q0, n: np.concatenate([random_run(rng, 1, query=q0 + k, db_id=k % 3) for k in range(n)])
    out["singletons"] = singles(0, 130)
    out["run_from_lane_63"] = np.concatenate([singles(0, 63), random_run(rng, 10, query=63), singles(64, 70)])
    out["long_run_from_lane_63"] = np.concatenate([singles(0, 63), random_run(rng, 70, query=63), singles(64, 3)])
    # many short runs side by side, of every length up to 70: the windows of the packed kernel cut them everywhere
    out["straddling"] = np.concatenate([random_run(rng, 1 + (7 * k) % 70, query=k // 4, db_id=k % 4) for k in range(60)])
    # a ladder: every hit precedes the next one, the chain is the run
    out["ladder"] = make([(12 * k, 10, 12 * k, 10) for k in range(150)], -1.0 - 0.01 * np.arange(150))
    return out


@pytest.fixture(scope="module")
def random_case():
    """runs of 1 to 300 hits, about 3,000 hits in all; with what chain_ref says of them, computed once"""
    rng = np.random.default_rng(7)
    lengths = [1, 300, 2, 64, 65, 200, 63, 128, 129, 17, 256, 1, 1, 90, 5, 33, 270, 40, 41, 150, 7, 100, 230, 3, 180, 75, 120, 12, 66, 57]
    hits = np.concatenate([random_run(rng, n, query=k // 3, db_id=k % 3) for k, n in enumerate(lengths)])
    return hits, keep_mask(hits)


def test_the_random_case_is_worth_running(random_case):
    hits, want = random_case
    assert 2500 <= len(hits) <= 3500
    chain_len = [len(m) for _, _, m, _ in chain_of_each_run(hits)]
    greedy = distinct_ref.keep_mask(hits)
    differs = sum(int((want[a:b] != greedy[a:b]).any()) for a, b in runs_of(hits))
    print("random case: hits", len(hits), "kept", int(want.sum()), "longest chain", max(chain_len), "runs where -u differs", differs)
    assert max(b - a for a, b in runs_of(hits)) > 64
    assert max(chain_len) >= 5 and sum(c >= 3 for c in chain_len) >= 10
    assert differs >= 1


def test_edges(ctx):
    from priblast_amd import capi
    assert len(capi.chain_sites(ctx, np.zeros(0, capi.HIT_DTYPE))) == 0
    for name, (hits, want) in expected_edges().items():
        assert keep_mask(hits).astype(int).tolist() == want, name  # (the yardstick itself)
        assert capi.chain_sites(ctx, hits).tolist() == want, name


def test_edges_by_the_workgroup_kernel(ctx, monkeypatch):
    from priblast_amd import capi
    monkeypatch.setenv("PRB_CHAIN_LDS_HITS", "1")
    for name, (hits, want) in expected_edges().items():
        assert capi.chain_sites(ctx, hits).tolist() == want, name


def test_boundaries(ctx):
    from priblast_amd import capi
    for name, hits in boundary_cases().items():
        want = keep_mask(hits)
        got = capi.chain_sites(ctx, hits)
        bad = np.flatnonzero(got != want.astype(np.uint8))
        assert len(bad) == 0, (name, len(hits), bad[:10].tolist())
        if name == "ladder":
            assert got.all()
        if name == "singletons":
            assert got.all()


@pytest.mark.parametrize("lds_hits", [None, "1", "40"])
def test_random_runs(ctx, random_case, monkeypatch, lds_hits):
    from priblast_amd import capi
    if lds_hits is not None:
        monkeypatch.setenv("PRB_CHAIN_LDS_HITS", lds_hits)
    hits, want = random_case
    ctx.reset_timers()
    got = capi.chain_sites(ctx, hits)
    bad = np.flatnonzero(got != want.astype(np.uint8))
    assert len(bad) == 0, (lds_hits, bad[:10].tolist())
    assert ctx.stage_ms("chain")[1] == 3 and ctx.stage_ms("distinct") == (0.0, 0)
    for a, b in runs_of(hits):  # every pair keeps a hit
        assert got[a:b].any()


def test_refusals(ctx):
    from priblast_amd import capi
    keep = np.zeros(4, np.uint8)
    assert capi.lib().prb_chain_sites(ctx.h, None, 4, keep.ctypes.data) == -1
    assert capi.lib().prb_chain_sites(ctx.h, None, -1, None) == -1
    assert capi.lib().prb_chain_sites(None, None, 0, None) == -1
    ok = make([(0, 5, 10, 5), (0, 5, 3, 5)], [-3.0, -3.0])
    with pytest.raises(capi.PrbError, match="hit 1 "):
        capi.chain_sites(ctx, ok)
    # ... but a lower db_sp that starts another run is fine
    ok["db_id"] = [0, 1]
    assert capi.chain_sites(ctx, ok).tolist() == [1, 1]
    three = np.concatenate([make([(0, 5, 10, 5), (0, 5, 10, 5)], [-3.0, -3.0]), make([(0, 5, 0, 5), (0, 5, 7, 5), (0, 5, 6, 5)], [-1.0] * 3, 1, 0)])
    with pytest.raises(capi.PrbError, match="hit 4 "):
        capi.chain_sites(ctx, three)
