"""GPU tests of the distinct-sites selection (launch_site_select) on hand-made lists of final hits, through
prb_distinct_sites: the greedy rule restated in distinct_ref.keep_mask is the yardstick.  Every case runs with the
build's LDS capacity and with PRB_DISTINCT_LDS_HITS forced small, which sends the runs of more than that many hits
to the workgroup kernel with their state in HBM (1: every run of two hits or more)."""
import numpy as np
import pytest

from distinct_ref import keep_mask

pytestmark = pytest.mark.gpu

LDS_HITS = 2048  # search_kernels.hpp, kSiteLdsHits


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


def random_run(rng, n, query=0, db_id=0, sort=True, span=None):
    """n rectangles over a field that grows with n (so that a hit meets a handful of others), energies from a coarse
    grid (many ties), sorted by db_sp as the search's list is - or not, as a caller's list may be"""
    span = span or max(40, 6 * n)
    db_sp = rng.integers(0, span, n)
    if sort:
        db_sp = np.sort(db_sp)
    rects = np.stack([rng.integers(0, 120, n), rng.integers(3, 40, n), db_sp, rng.integers(3, 40, n)], axis=1)
    return make(rects, -8.0 - 0.5 * rng.integers(0, 12, n), query, db_id)


def chain(n, descending):
    """neighbours intersect, nobody else does; the energy falls (or rises) along the run, so hit k waits for hit k + 1
    (or k - 1): as many rounds as hits"""
    rects = [(5 * k, 10, 5 * k, 10) for k in range(n)]
    e = -8.0 - 0.01 * np.arange(n)
    return make(rects, e if descending else e[::-1].copy())


def cases():
    rng = np.random.default_rng(3)
    out = {}
    for n in (1, 2, 63, 64, 65, 1025):
        out[f"run{n}"] = random_run(rng, n)
        out[f"run{n}_unsorted"] = random_run(rng, n, sort=False)
    out["dense65"] = random_run(rng, 65, span=60)  # everything meets nearly everything
    out["beyond_lds"] = random_run(rng, LDS_HITS + 452)
    singles = lambda q0, n: np.concatenate([random_run(rng, 1, query=q0 + k, db_id=k % 3) for k in range(n)])
    out["singletons_long_singletons"] = np.concatenate([singles(0, 200), random_run(rng, 300, query=200), singles(201, 200)])
    # many short runs side by side, of every length up to 70: the windows of the packed kernel cut them everywhere
    out["packed"] = np.concatenate([random_run(rng, 1 + (7 * k) % 70, query=k // 4, db_id=k % 4) for k in range(160)])
    out["chain_descending"] = chain(300, True)
    out["chain_ascending"] = chain(300, False)
    return out


def expected_edges():
    """(list, keep) pairs that spell the rule out"""
    e = [-10.0, -9.0]
    return {
        "touch": (make([(0, 10, 0, 10), (9, 10, 9, 10)], e), [1, 0]),           # end == start: one shared position
        "adjacent": (make([(0, 10, 0, 10), (10, 10, 10, 10)], e), [1, 1]),      # end + 1 == start: none
        "query_only": (make([(0, 10, 0, 10), (5, 10, 50, 10)], e), [1, 1]),
        "target_only": (make([(0, 10, 0, 10), (50, 10, 5, 10)], e), [1, 1]),
        "tie_place": (make([(0, 10, 0, 10), (5, 10, 5, 10)], [-9.0, -9.0]), [1, 0]),
        "tie_place_three": (make([(0, 10, 0, 10), (5, 10, 5, 10), (12, 10, 12, 10)], [-9.0] * 3), [1, 0, 1]),
        "zeros": (make([(0, 10, 0, 10), (5, 10, 5, 10)], [0.0, -0.0]), [1, 0]),  # -0.0 is not better than +0.0
        "zeros_swapped": (make([(0, 10, 0, 10), (5, 10, 5, 10)], [-0.0, 0.0]), [1, 0]),
        # A better than B better than C; A meets B, B meets C, A does not meet C: B is dropped and suppresses nothing
        "greedy": (make([(0, 10, 0, 10), (8, 10, 8, 10), (16, 10, 16, 10)], [-12.0, -11.0, -10.0]), [1, 0, 1]),
        "greedy_mixed": (make([(16, 10, 16, 10), (8, 10, 8, 10), (0, 10, 0, 10)], [-10.0, -11.0, -12.0]), [1, 0, 1]),
        "pairs_apart": (np.concatenate([make([(0, 10, 0, 10)], [-9.0], 0, 0), make([(0, 10, 0, 10)], [-8.0], 0, 1),
                                        make([(0, 10, 0, 10)], [-8.0], 1, 1)]), [1, 1, 1]),
    }


@pytest.mark.parametrize("lds_hits", [None, "1", "8"])
def test_selection_equals_the_greedy_rule(ctx, monkeypatch, lds_hits):
    from priblast_amd import capi
    if lds_hits is not None:
        monkeypatch.setenv("PRB_DISTINCT_LDS_HITS", lds_hits)
    assert len(capi.distinct_sites(ctx, np.zeros(0, capi.HIT_DTYPE))) == 0
    for name, (hits, want) in expected_edges().items():
        assert keep_mask(hits).astype(int).tolist() == want, name  # (the yardstick itself)
        assert capi.distinct_sites(ctx, hits).tolist() == want, (name, lds_hits)
    dropped = 0
    for name, hits in cases().items():
        want = keep_mask(hits)
        got = capi.distinct_sites(ctx, hits)
        bad = np.flatnonzero(got != want.astype(np.uint8))
        assert len(bad) == 0, (name, lds_hits, len(hits), bad[:10].tolist())
        dropped += int((~want).sum())
    assert dropped > 1000  # (the cases do suppress)


def test_chains_alternate(ctx):
    """the worst case for rounds, spelled out: from the best end of the chain every second hit is kept"""
    from priblast_amd import capi
    n = 300
    assert capi.distinct_sites(ctx, chain(n, True)).tolist() == [(n - 1 - k) % 2 == 0 for k in range(n)]
    assert capi.distinct_sites(ctx, chain(n, False)).tolist() == [k % 2 == 0 for k in range(n)]


def test_refusals(ctx):
    from priblast_amd import capi
    keep = np.zeros(4, np.uint8)
    assert capi.lib().prb_distinct_sites(ctx.h, None, 4, keep.ctypes.data) == -1
    assert capi.lib().prb_distinct_sites(ctx.h, None, -1, None) == -1
    assert capi.lib().prb_distinct_sites(None, None, 0, None) == -1
