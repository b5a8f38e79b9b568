"""Hand-spelled hit lists for the tests of the stages' sort and redundancy filter (test_sortfilter_ref.py pins the
oracle's orc_sort_filter to them, test_gpu_sort_filter.py runs them through prb_sort_filter).

The order: db_sp and q_sp ascending, db_len and q_len descending, then e_tot, e_hyb, e_acc ascending, then the input
order.  The sweep (CheckRedundancy): a hit above the threshold is dropped and scans nothing; an unflagged hit a scans the
unflagged hits b behind it while b.db_sp <= a's db end, and where a's query range contains b's and a's db end >= b's,
a is flagged if E_a > E_b, else b."""
import numpy as np

from priblast_amd.capi import HIT_DTYPE

THR = -6.0


def H(q_sp, q_len, db_sp, db_len, e_tot, e_hyb=None, e_acc=0.0, query=0, db_id=0):
    return (q_sp, db_sp, q_len, db_len, db_id, 0, e_acc, e_tot if e_hyb is None else e_hyb, e_tot, query, 0, 0)


def hits_of(rows):
    return np.array(rows, HIT_DTYPE)


BOX = (0, 10, 0, 10)       # q 0..9, db 0..9
BIG = (0, 20, 0, 20)       # q 0..19, db 0..19: contains IN
IN = (5, 5, 5, 5)          # q 5..9, db 5..9
U1 = (0, 30, 0, 30)        # q 0..29, db 0..29: contains B3, not U2
U2 = (3, 40, 2, 20)        # q 3..42, db 2..21: contains B3
B3 = (5, 5, 5, 5)
over = np.nextafter(THR, np.inf)


def edges():
    """name -> (rows, threshold, order: index in rows of the hit at each sorted place, keep by sorted place)"""
    c = {
        # identical boxes, equal energy: the earlier one (lower e_hyb) scans the other and the `else` branch flags it
        "identical_equal": ([H(*BOX, -8.0, -7.0), H(*BOX, -8.0, -9.0)], THR, [1, 0], [1, 0]),
        "container_lower": ([H(*BIG, -9.0), H(*IN, -8.0)], THR, [0, 1], [1, 0]),
        "container_higher": ([H(*BIG, -7.0), H(*IN, -8.0)], THR, [0, 1], [0, 1]),
        "container_equal": ([H(*BIG, -8.0), H(*IN, -8.0)], THR, [0, 1], [1, 0]),
        # the query range is contained, the database interval lies in front of the container's: no relation
        "query_only": ([H(0, 20, 5, 20, -9.0), H(5, 5, 0, 5, -8.0)], THR, [1, 0], [1, 1]),
        # ... or overlaps it and ends behind it (db 5..24 against 0..9): no relation
        "query_only_shorter_db_end": ([H(0, 20, 0, 10, -9.0), H(5, 5, 5, 20, -8.0)], THR, [0, 1], [1, 1]),
        "at_threshold": ([H(*BOX, THR)], THR, [0], [1]),
        "just_above_threshold": ([H(*BOX, over)], THR, [0], [0]),
        "over_contains_good": ([H(*BIG, -5.0), H(*IN, -8.0)], THR, [0, 1], [0, 1]),
        # the container's scan reaches the hit above the threshold before the sweep does: E_a > E_b is false, b is flagged
        "good_contains_over": ([H(*BIG, -8.0), H(*IN, -5.0)], THR, [0, 1], [1, 0]),
        # compare()'s four fields
        "cmp_db_sp": ([H(0, 5, 7, 5, -8.0), H(0, 5, 3, 5, -8.0)], THR, [1, 0], [1, 1]),
        "cmp_q_sp": ([H(9, 5, 3, 5, -8.0), H(2, 5, 3, 5, -8.0)], THR, [1, 0], [1, 1]),
        "cmp_db_len_desc": ([H(2, 5, 3, 5, -8.0), H(2, 5, 3, 9, -7.0)], THR, [1, 0], [0, 1]),
        "cmp_q_len_desc": ([H(2, 5, 3, 9, -8.0), H(2, 8, 3, 9, -9.0)], THR, [1, 0], [1, 0]),
        # each field outweighs the ones behind it: db_sp over q_sp, q_sp over db_len, db_len over q_len
        "cmp_priority": ([H(4, 9, 5, 9, -8.0), H(9, 3, 2, 3, -8.0), H(4, 3, 5, 12, -8.0), H(1, 2, 5, 2, -8.0)], THR,
                         [1, 3, 2, 0], [1, 1, 1, 1]),
        # the tie-break fields
        "tie_e_tot": ([H(*BOX, -7.0), H(*BOX, -9.0)], THR, [1, 0], [1, 0]),
        "tie_e_hyb": ([H(*BOX, -8.0, -7.0), H(*BOX, -8.0, -9.0)], THR, [1, 0], [1, 0]),
        "tie_e_acc": ([H(*BOX, -8.0, -9.0, 1.0), H(*BOX, -8.0, -9.0, 0.5)], THR, [1, 0], [1, 0]),
        "tie_e_tot_over_e_hyb": ([H(*BOX, -8.0, -20.0), H(*BOX, -9.0, -1.0)], THR, [1, 0], [1, 0]),
        "tie_e_hyb_over_e_acc": ([H(*BOX, -8.0, -9.0, 0.1), H(*BOX, -8.0, -10.0, 0.9)], THR, [1, 0], [1, 0]),
        "tie_input_order": ([H(*BOX, -8.0, db_id=1), H(*BOX, -8.0, db_id=2), H(*BOX, -8.0, db_id=3)], THR, [0, 1, 2], [1, 0, 0]),
        # U1 is active and flags b; U2 between them contains b, E_U2 > E_b, but b is flagged already: U2 survives
        "already_flagged": ([H(*U1, -9.0), H(*U2, -7.0), H(*B3, -8.0)], THR, [0, 1, 2], [1, 1, 0]),
        # U1 above the threshold flags nothing: U2's scan meets b unflagged and flags U2
        "already_flagged_u1_over": ([H(*U1, -5.0), H(*U2, -7.0), H(*B3, -8.0)], THR, [0, 1, 2], [0, 0, 1]),
    }
    c.update(zeros())
    return c


def zeros():
    """+0.0 against -0.0 in each energy field: equal for the comparator, so the next field decides (an order by bit
    pattern would put -0.0 first: the other order in every case here).  Thresholds 0.0 and 1.0: neither hit is above."""
    c = {}
    for thr in (0.0, 1.0):
        t = f"_thr{thr:g}"
        c["zero_e_tot" + t] = ([H(*BOX, -0.0, -1.0), H(*BOX, 0.0, -2.0)], thr, [1, 0], [1, 0])
        c["zero_e_tot_swapped" + t] = ([H(*BOX, 0.0, -2.0), H(*BOX, -0.0, -1.0)], thr, [0, 1], [1, 0])
        c["zero_e_hyb" + t] = ([H(*BOX, 0.0, -0.0, 2.0), H(*BOX, 0.0, 0.0, 1.0)], thr, [1, 0], [1, 0])
        c["zero_e_acc" + t] = ([H(*BOX, 0.0, 0.0, 0.0, db_id=1), H(*BOX, 0.0, 0.0, -0.0, db_id=2)], thr, [0, 1], [1, 0])
        # as the contained hit: E_a > E_b is false between the zeros, so b is flagged whichever sign it has
        c["zero_contained" + t] = ([H(*BIG, 0.0), H(*IN, -0.0)], thr, [0, 1], [1, 0])
        c["zero_container" + t] = ([H(*BIG, -0.0), H(*IN, 0.0)], thr, [0, 1], [1, 0])
    return c
