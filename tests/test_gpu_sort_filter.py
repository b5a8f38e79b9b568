"""GPU tests of the stages' sort (sort_hits, sort_kernels.hip) and redundancy filter (filter_hits, filter_kernels.hip) on
hand-made lists, through prb_sort_filter.  The yardstick is oraclelib.sort_filter: the oracle's own comparator and sweep
(test_sortfilter_ref.py spells it out).  Every case runs with the default forms, with the plain filter kernels
(PRB_FILTER_TILES=0), with the sort field by field (PRB_SORT_FOUR_KEYS) and with the two-length key forced
(PRB_SORT_TWO_LENGTHS), and every form must equal the oracle.

The tiled filter kernels hold a window of the sorted list in LDS: 128 hits in front of a tile of 256 and (final pass)
128 behind it; the tie pass of the one-key sort takes runs of up to 4096 hits with identical coordinates.  The cases put
list lengths, query boundaries, container-to-contained distances and run lengths on and around those numbers."""
import functools

import numpy as np
import pytest

import oraclelib
import sortfilter_cases as sc

pytestmark = pytest.mark.gpu

THR = sc.THR
KNOBS = {"default": None, "plain_filter": ("PRB_FILTER_TILES", "0"), "four_keys": ("PRB_SORT_FOUR_KEYS", "1"),
         "two_lengths": ("PRB_SORT_TWO_LENGTHS", "1")}
INTS = ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start", "query", "bp_count", "bp_offset")
ENERGIES = ("e_acc", "e_hyb", "e_tot")
TWO, ONE, WIDTH, TIE_RUN, FORCED = range(5)  # capi.SORT_*


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(params=sorted(KNOBS))
def knob(request, monkeypatch):
    if KNOBS[request.param]:
        monkeypatch.setenv(*KNOBS[request.param])
    return request.param


def packed_form(h):
    """the one-key sort's form for a list whose key fits: the length once when every hit has q_len == db_len"""
    return ONE if (h["q_len"] == h["db_len"]).all() else TWO


def form_under(knob, base):
    """the form the sort reports for a list that takes `base` by default"""
    if knob == "four_keys":
        return FORCED
    return TWO if (knob == "two_lengths" and base == ONE) else base


# ---------------------------------------------------------------------------------------------------- lists
def random_list(rng, n, query=0, one_len=False):
    """n hits whose database starts spread over n / 2 positions (a hit meets a handful of others), lengths 5..39,
    energies on a grid of 0.5 from -4 to -9.5 (a third above the threshold of -6, many ties), in no order"""
    h = np.zeros(n, sc.HIT_DTYPE)
    h["db_sp"] = rng.integers(0, max(n // 2, 1), n)
    h["q_sp"] = rng.integers(0, 120, n)
    h["q_len"] = rng.integers(5, 40, n)
    h["db_len"] = h["q_len"] if one_len else rng.integers(5, 40, n)
    h["e_tot"] = -4.0 - 0.5 * rng.integers(0, 12, n)
    h["e_acc"] = 0.5 * rng.integers(0, 4, n)
    h["e_hyb"] = h["e_tot"] - h["e_acc"]
    h["db_id"] = rng.integers(0, 50, n)
    h["db_id_start"] = rng.integers(0, 1000, n)
    h["query"] = query
    return h


def fillers(positions, query=0):
    """one hit per position (= its db_sp, so also its place in a sorted list whose db_sp are all distinct) that contains
    no other filler and lies outside the query range 0..299 of the umbrellas: q 300 + 7 * (p % 50) .. + 4, db p .. p + 4"""
    p = np.asarray(positions, np.int64)
    h = np.zeros(len(p), sc.HIT_DTYPE)
    h["db_sp"], h["q_sp"] = p, 300 + 7 * (p % 50)
    h["q_len"] = h["db_len"] = 5
    h["e_tot"] = h["e_hyb"] = -7.0
    h["query"] = query
    return h


def placed(n, special, query=0):
    """a list of n hits for one query: special = {place: row of sortfilter_cases.H without db_sp}, fillers elsewhere"""
    rest = [p for p in range(n) if p not in special]
    rows = [sc.H(r[0], r[1], p, r[2], *r[3:], query=query) for p, r in special.items()]
    return np.concatenate([sc.hits_of(rows), fillers(rest, query)])


DISTANCES = (100, 127, 128, 129, 300, 383, 384, 385, 700, 2000)


def umbrella_list(e_umbrella, e_inner, two=False, query=0):
    """an umbrella (q 0..199, db 0..4999) at place 0 - with `two`, a second one (q 0..149, db 1..4000) at place 1, which
    the first contains - and hits both contain at the DISTANCES behind the first; e_inner: their energies in turn"""
    special = {0: (0, 200, 5000, e_umbrella)}
    if two:
        special[1] = (0, 150, 4000, e_umbrella + 0.5)
    for k, d in enumerate(DISTANCES):
        special[d] = (10 + 6 * k, 5, 5, e_inner[k % len(e_inner)])
    return placed(DISTANCES[-1] + 40, special, query)


def triple_list(p1, p2, pb, e1, query=0):
    """sortfilter_cases' already-flagged triple at the places p1 < p2 < pb: U1 (q 0..199) flags b (q 60..64) unless it is
    above the threshold; U2 (q 50..249, not contained in U1) contains b with E_U2 > E_b"""
    return placed(pb + 300, {p1: (0, 200, 5000, e1), p2: (50, 200, 4000, -7.0), pb: (60, 5, 5, -8.0)}, query)


def tie_run(rng, n, q_sp, db_sp):
    """n hits with identical coordinates: three values of each energy, one of e_tot above the threshold, so that
    every tie-break field decides somewhere and many records are identical in every field"""
    h = np.zeros(n, sc.HIT_DTYPE)
    h["q_sp"], h["db_sp"], h["q_len"], h["db_len"] = q_sp, db_sp, 30, 35
    h["e_tot"] = rng.choice([-8.0, -7.5, -5.0], n)
    h["e_hyb"] = rng.choice([-9.0, -8.5, -8.0], n)
    h["e_acc"] = rng.choice([0.5, 1.0, 1.5], n)
    return h


def shuffled(rng, h):
    return h[rng.permutation(len(h))]


SIZES = (0, 1, 2, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 1025)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (hits, threshold, the form the default sort must report or None, the oracle's records, its keep flags);
    built, and the oracle run, once for all forms"""
    rng = np.random.default_rng(11)
    c = {}
    for n in SIZES:
        c[f"size{n}"] = (shuffled(rng, random_list(rng, n)), THR, "packed" if n else None)
        # five queries: boundaries at 255, 512, 769 and 1024 - one in front of a tile edge, on one, one behind one, on one
        parts = [random_list(rng, m, q) for m, q in zip((255, 257, 257, 255, n), (3, 4, 6, 7, 9))]
        c[f"size{n}_fifth_query"] = (shuffled(rng, np.concatenate(parts)), THR, TWO)
    for n in (300, 1000, 3000, 12000):
        c[f"random{n}"] = (shuffled(rng, random_list(rng, n)), THR, TWO)
    below, equal, above, mixed = (-8.0,), (-9.0,), (-9.5,), (-9.5, -8.0, -9.0)
    for two in (False, True):
        for name, e_u, e_in in (("below", -9.0, below), ("equal", -9.0, equal), ("above", -9.0, above), ("mixed", -9.0, mixed),
                                ("over", -5.0, below)):
            c[f"umbrella{1 + two}_{name}"] = (shuffled(rng, umbrella_list(e_u, e_in, two)), THR, TWO)
    front = lambda: random_list(rng, 300, query=1)  # a query in front: the running maximum of the end keys starts high
    behind = lambda: random_list(rng, 200, query=5)
    c["umbrella_second_query"] = (shuffled(rng, np.concatenate([front(), umbrella_list(-9.0, mixed, True, 2), behind()])), THR, TWO)
    # U1, U2, b: more than 384 apart; in neighbouring tiles; within one window; on both sides of a tile edge; b past the
    # forward window of U2's tile; U1 past the backward window of U2's tile
    for places in ((0, 400, 800), (200, 300, 520), (250, 260, 300), (255, 256, 257), (100, 500, 640), (0, 130, 390),
                   (100, 511, 900), (3, 1000, 2000)):
        for e1, tag in ((-9.0, ""), (-5.0, "_u1_over")):
            name = "triple_%d_%d_%d%s" % (*places, tag)
            c[name] = (shuffled(rng, triple_list(*places, e1)), THR, TWO)
            c[name + "_second_query"] = (shuffled(rng, np.concatenate([front(), triple_list(*places, e1, query=2), behind()])), THR, TWO)
    c["ties_small"] = (shuffled(rng, np.concatenate([random_list(rng, 400), tie_run(rng, 2, 7, 20), tie_run(rng, 3, 50, 90),
                                                     tie_run(rng, 64, 20, 150)])), THR, TWO)
    c["ties_4096"] = (shuffled(rng, np.concatenate([random_list(rng, 400), tie_run(rng, 4096, 20, 100)])), THR, TWO)
    c["ties_4097"] = (shuffled(rng, np.concatenate([random_list(rng, 400), tie_run(rng, 4097, 20, 100)])), THR, TIE_RUN)
    c["ties_4097_second_query"] = (shuffled(rng, np.concatenate([front(), random_list(rng, 300, 2), tie_run(rng, 4097, 20, 100)])), THR,
                                   TIE_RUN)
    wide = random_list(rng, 600)
    wide["db_sp"] = 2**30 - rng.integers(0, 300, 600)
    wide["q_sp"] = rng.integers(0, 100000, 600) // 20000 * 20000 + rng.integers(0, 40, 600)
    wide["q_len"], wide["db_len"] = rng.integers(59000, 60100, 600), rng.integers(59000, 60100, 600)
    wide["query"] = rng.choice([0, 5, 2**20 - 1, 2**20], 600)
    c["key_too_wide"] = (wide, THR, WIDTH)
    same = shuffled(rng, random_list(rng, 700, one_len=True))
    c["one_length"] = (same, THR, ONE)
    changed = same.copy()
    changed["db_len"][123] += 1
    c["one_length_but_one_hit"] = (changed, THR, TWO)
    for name, (rows, thr, _, _) in sc.edges().items():
        h = sc.hits_of(rows)
        c["edge_" + name] = (h, thr, "packed")
    return {name: (h, thr, packed_form(h) if form == "packed" else form) + oraclelib.sort_filter(h, thr) for name, (h, thr, form) in c.items()}


def same_records(got, want):
    """field by field, energies as bit patterns but for the sign of a zero"""
    for f in INTS:
        if not np.array_equal(got[f], want[f]):
            return f, np.flatnonzero(got[f] != want[f])[:5].tolist()
    for f in ENERGIES:
        a, b = (got[f] + 0.0).view(np.uint64), (want[f] + 0.0).view(np.uint64)
        if not np.array_equal(a, b):
            return f, np.flatnonzero(a != b)[:5].tolist()
    return None


def run_case(ctx, name, knob):
    from priblast_amd import capi
    hits, thr, form, want, want_keep = cases()[name]
    got, keep, got_form = capi.sort_filter(ctx, hits, thr)
    assert same_records(got, want) is None, (name, knob, len(hits), same_records(got, want))
    bad = np.flatnonzero(keep != want_keep)
    assert len(bad) == 0, (name, knob, len(hits), bad[:10].tolist(), want_keep[bad[:10]].tolist())
    assert got_form == (None if form is None else form_under(knob, form)), (name, knob, got_form)
    return got, keep


def run_group(ctx, prefix, knob, at_least):
    names = [n for n in cases() if n.startswith(prefix)]
    assert len(names) >= at_least, names
    for name in names:
        run_case(ctx, name, knob)


# ---------------------------------------------------------------------------------------------------- tests
def test_hand_spelled_edges(ctx, knob):
    """the lists of test_sortfilter_ref.py, the +0.0 / -0.0 ones with thresholds 0.0 and 1.0 among them: the expected
    order and flags are the literals there (the oracle equals them; checked again here, the GPU against both)"""
    edges = sc.edges()
    for name, (rows, thr, order, keep) in edges.items():
        got, got_keep = run_case(ctx, "edge_" + name, knob)
        assert same_records(got, sc.hits_of(rows)[order]) is None, (name, knob)
        assert got_keep.tolist() == keep, (name, knob)


def test_sizes_and_query_boundaries(ctx, knob):
    run_group(ctx, "size", knob, 2 * len(SIZES))


@functools.lru_cache(maxsize=None)
def drop_kinds(name):
    """(above the threshold, contained, containers that flagged themselves, survivors) of a case, from the oracle's own
    answers.  What earlier hits do to a hit does not depend on the hits behind it, and a hit flags itself only over a hit
    behind it: a hit that is not above the threshold is dropped as contained iff the oracle drops it as the LAST hit of
    the list cut behind it.  (Counted up to 10 of each kind: the cuts are short.)"""
    _, thr, _, recs, keep = cases()[name]
    over = recs["e_tot"] > thr
    contained = itself = 0
    for j in np.flatnonzero(~over & (keep == 0)):
        if oraclelib.sort_filter(recs[:j + 1], thr)[1][j] == 0:
            contained += 1
        else:
            itself += 1
        if contained >= 10 and itself >= 10:
            break
    return int(over.sum()), contained, itself, int(keep.sum())


@pytest.mark.parametrize("n", [300, 1000, 3000, 12000])
def test_random_lists(ctx, knob, n):
    kinds = drop_kinds(f"random{n}")
    assert min(kinds) >= 10, (n, kinds)  # (a generator that empties a class would leave the case checking less)
    run_case(ctx, f"random{n}", knob)


def test_umbrella_distances(ctx, knob):
    """container and contained hit 100 .. 2000 places apart, fillers between them: the scans leave the LDS window"""
    for name in ("umbrella1_below", "umbrella1_equal", "umbrella2_mixed"):  # (the lists do what they are built for)
        _, _, _, recs, keep = cases()[name]
        inner = recs["q_sp"] < 300
        assert keep[~inner].all() and int(inner.sum()) == len(DISTANCES) + 1 + name.startswith("umbrella2")
    _, _, _, recs, keep = cases()["umbrella1_below"]
    assert keep[0] == 1 and not keep[list(DISTANCES)].any()
    _, _, _, recs, keep = cases()["umbrella1_above"]
    assert keep[0] == 0 and keep[list(DISTANCES)].all()
    run_group(ctx, "umbrella", knob, 11)


def test_already_flagged_triples(ctx, knob):
    """the backward scan inside the final pass ("was b flagged by an active hit before a") across windows and tiles"""
    for places in ((0, 400, 800), (255, 256, 257)):
        p1, p2, pb = places
        assert cases()["triple_%d_%d_%d" % places][4][[p1, p2, pb]].tolist() == [1, 1, 0]
        assert cases()["triple_%d_%d_%d_u1_over" % places][4][[p1, p2, pb]].tolist() == [0, 0, 1]
    run_group(ctx, "triple", knob, 32)


def test_tie_runs(ctx, knob):
    """runs of identical coordinates of 2, 3, 64, 4096 (the longest the tie pass takes) and 4097 hits (the sort starts
    over field by field); run_case checks the reported form"""
    run_group(ctx, "ties", knob, 4)


def test_key_forms(ctx, knob):
    for name in ("key_too_wide", "one_length", "one_length_but_one_hit"):
        run_case(ctx, name, knob)


def test_order_independence(ctx, knob):
    """shuffles of one list - identical records, tie runs and several queries in it - and the list as two halves that
    arrive in either order, one of them reversed: the same records and flags"""
    from priblast_amd import capi
    rng = np.random.default_rng(5)
    base = np.concatenate([random_list(rng, 700, 2), random_list(rng, 300, 4), tie_run(rng, 40, 20, 100), tie_run(rng, 40, 20, 100)])
    base = np.concatenate([base, base[:50]])
    half = len(base) // 2
    orders = [shuffled(rng, base) for _ in range(3)] + [np.concatenate([base[half:], base[:half]]),
                                                       np.concatenate([base[:half][::-1], base[half:]])]
    want, want_keep = oraclelib.sort_filter(base, THR)
    for k, h in enumerate(orders):
        got, keep, _ = capi.sort_filter(ctx, h, THR)
        assert same_records(got, want) is None, (k, knob, same_records(got, want))
        assert np.array_equal(keep, want_keep), (k, knob)


def test_refusals(ctx):
    from priblast_amd import capi
    L = capi.lib()
    h = random_list(np.random.default_rng(1), 4)
    out, keep, form = np.zeros(4, sc.HIT_DTYPE), np.zeros(4, np.uint8), np.zeros(1, np.int32)
    args = lambda hits: (hits.ctypes.data, 4, THR, out.ctypes.data, keep.ctypes.data, form.ctypes.data)
    assert L.prb_sort_filter(ctx.h, *args(h)) == 0
    assert L.prb_sort_filter(None, *args(h)) == -1
    assert L.prb_sort_filter(ctx.h, None, 4, THR, out.ctypes.data, keep.ctypes.data, form.ctypes.data) == -1
    assert L.prb_sort_filter(ctx.h, h.ctypes.data, 4, THR, None, keep.ctypes.data, form.ctypes.data) == -1
    assert L.prb_sort_filter(ctx.h, h.ctypes.data, 4, THR, out.ctypes.data, None, form.ctypes.data) == -1
    assert L.prb_sort_filter(ctx.h, None, -1, THR, None, None, None) == -1
    assert L.prb_sort_filter(ctx.h, h.ctypes.data, 2**31, THR, out.ctypes.data, keep.ctypes.data, form.ctypes.data) == -1
    assert L.prb_sort_filter(None, None, 0, THR, None, None, None) == -1
    assert L.prb_sort_filter(ctx.h, None, 0, THR, None, None, None) == 0
    bad = h.copy()
    bad["query"][2] = -1
    assert L.prb_sort_filter(ctx.h, *args(bad)) == -1
    assert b"query" in L.prb_last_error()
