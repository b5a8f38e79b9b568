"""tests/eval_ref.py - the restatement that the GPU tests of the evalset compare with - pinned on hand-worked cases
(no GPU).  Every expected figure below is worked out by hand from the definitions in include/priblast_hip.h."""
from fractions import Fraction

import numpy as np

import eval_ref


def figures(recs):
    return [(int(r["null_le"]), int(r["rank"]), int(r["q_num"]), int(r["q_den"])) for r in recs]


def test_a_query_without_real_hits_has_no_records():
    assert len(eval_ref.score_query([], [-9.0, -12.0], 3)) == 0
    out = eval_ref.score(2, [1], [-9.0], [0, 0], [-10.0, -11.0], 3)
    assert figures(out) == [(0, 1, 0, 1)]  # (query 0's decoys are not query 1's)


def test_without_decoy_hits_every_null_le_is_zero_and_every_q_is_zero_over_the_own_rank():
    out = eval_ref.score_query([-10.0, -12.0, -9.0], [], 2)
    assert figures(out) == [(0, 2, 0, 2), (0, 1, 0, 1), (0, 3, 0, 3)]
    assert list(out["decoys"]) == [2, 2, 2]
    assert list(eval_ref.evalue(out)) == [0, 0, 0] and list(eval_ref.qvalue(out)) == [0, 0, 0]


def test_a_decoy_of_equal_energy_is_counted():
    out = eval_ref.score_query([-10.0], [-10.0, -9.0], 1)
    assert figures(out) == [(1, 1, 1, 1)]  # 1 / (1 * 1) = 1: not above 1, the hit's own pair
    # ... and so is a real hit of equal energy: both share rank 2; -0.0 is +0.0
    out = eval_ref.score_query([-7.0, -7.0, -0.0], [0.0], 4)
    assert figures(out) == [(0, 2, 0, 2), (0, 2, 0, 2), (1, 3, 1, 3)]


def test_of_equal_fractions_the_lowest_energy_is_kept():
    # M = 1.  real -20 -18 -16 -14, decoys -19 -17: FDR = 0/1, 1/2, 2/3, 2/4 from the lowest energy up
    out = eval_ref.score_query([-14.0, -16.0, -18.0, -20.0], [-19.0, -17.0], 1)
    assert figures(out) == [(2, 4, 2, 4), (2, 3, 2, 4), (1, 2, 1, 2), (0, 1, 0, 1)]
    # (-18's minimum is 1/2 = 2/4: its own pair, not the one of -14)


def test_a_minimum_above_one_is_stored_as_m_over_one():
    out = eval_ref.score_query([-10.0], [-12.0, -11.0, -10.5, -13.0, -10.0], 2)
    assert figures(out) == [(5, 1, 2, 1)]
    assert list(eval_ref.qvalue(out)) == [1.0] and list(eval_ref.evalue(out)) == [2.5]
    # 2/2 is not above 1: the pair stays
    assert figures(eval_ref.score_query([-10.0], [-12.0, -11.0], 2)) == [(2, 1, 2, 1)]


def test_a_positive_energy_beside_negative_ones():
    out = eval_ref.score_query([2.5, -3.0], [1.0, -5.0], 2)
    assert figures(out) == [(2, 2, 2, 2), (1, 1, 1, 1)]  # -3: min(1/2, 2/4), equal: its own
    out = eval_ref.score_query([2.5, -3.0, 0.5], [1.0, -5.0], 2)
    assert figures(out) == [(2, 3, 2, 3), (1, 1, 1, 2), (1, 2, 1, 2)]  # -3: min(1/2, 1/4, 2/6) = 1/4, of 0.5


def test_the_q_value_never_falls_as_the_energy_rises_and_matches_the_definition():
    rng = np.random.default_rng(5)
    for _ in range(30):
        m = int(rng.integers(1, 5))
        real = np.round(rng.normal(-10, 3, int(rng.integers(1, 40))), 1)  # (rounded: equal energies occur)
        decoy = np.round(rng.normal(-8, 3, int(rng.integers(0, 60))), 1)
        out = eval_ref.score_query(real, decoy, m)
        order = np.argsort(real, kind="stable")
        q = [Fraction(int(out["q_num"][i]), m * int(out["q_den"][i])) for i in order]
        assert all(a <= b for a, b in zip(q, q[1:]))
        for i in range(len(real)):  # the definition, literally
            fdr = [Fraction(int(np.sum(decoy <= real[g])), m * int(np.sum(real <= real[g]))) for g in range(len(real)) if real[g] >= real[i]]
            assert Fraction(int(out["q_num"][i]), m * int(out["q_den"][i])) == min(1, min(fdr))


def test_score_looks_hits_up_by_query_and_energy():
    out = eval_ref.score(2, [0, 1, 0], [-10.0, -10.0, -8.0], [1, 0], [-11.0, -9.0], 1, look_q=[0, 1], look_e=[-8.0, -10.0])
    assert figures(out) == [(1, 2, 1, 2), (1, 1, 1, 1)]
