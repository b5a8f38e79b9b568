"""The yardstick of test_gpu_sort_filter.py, on the CPU: oraclelib.sort_filter (orc_sort_filter: the oracle's own hit_cmp
and CheckRedundancy sweep, pinned to the reference by the stage dumps) against lists of one to four hits whose order
and keep flags are written out by hand (sortfilter_cases.edges)."""
import numpy as np
import pytest

import oraclelib
from sortfilter_cases import BOX, THR, H, edges, hits_of

EDGES = edges()


def records_equal(a, b):
    return all(np.array_equal(a[f].view(np.uint64) if a[f].dtype.kind == "f" else a[f], b[f].view(np.uint64) if b[f].dtype.kind == "f" else b[f])
               for f in a.dtype.names)


@pytest.mark.parametrize("name", sorted(EDGES))
def test_hand_spelled(name):
    rows, thr, order, keep = EDGES[name]
    hits = hits_of(rows)
    got, got_keep = oraclelib.sort_filter(hits, thr)
    assert records_equal(got, hits[order]), (name, got)
    assert got_keep.tolist() == keep, name


def test_queries_are_lists_of_their_own():
    """a container in another query flags nothing; the parts come back in query order, each sorted"""
    big, inner = (0, 20, 0, 20), (5, 5, 5, 5)
    hits = hits_of([H(*inner, -8.0, query=4), H(*big, -9.0, query=2), H(*inner, -8.0, query=2), H(*big, -7.0, query=4),
                    H(*BOX, -5.0, query=0)])
    got, keep = oraclelib.sort_filter(hits, THR)
    assert records_equal(got, hits[[4, 1, 2, 3, 0]])
    assert keep.tolist() == [0, 1, 0, 0, 1]


def test_input_is_left_alone_and_empty_lists_pass():
    hits = hits_of(EDGES["already_flagged"][0])
    before = hits.copy()
    oraclelib.sort_filter(hits, THR)
    assert records_equal(hits, before)
    got, keep = oraclelib.sort_filter(hits[:0], THR)
    assert len(got) == 0 and len(keep) == 0
