"""The pairs of the one-pass seed path (k_pair_key, the radix sort, k_seed_extend) in their two layouts and with the
order of a tile made in LDS: whatever the layout, the bits the radix sort covers and the chunking, stages 1 - 3 give the
hits, base pairs and counts of the search in suffix-array order (PRB_SEED_ROW_SHIFT=-1, the reference's emission order,
which takes no pair sort at all) bit for bit - the sort behind the seeds is total on the hits' own fields.  And the
choice of the layout itself (prb_seed_pair_layout), on the host."""
import os

import numpy as np
import pytest

import refdump
from test_gpu_pairlist import make_mask, search, tbase_of
from test_gpu_tophits import open_batch

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOBS = ("PRB_SEARCH_CHUNK_PAIRS", "PRB_SEED_FUSED", "PRB_SEED_ROW_SHIFT", "PRB_NO_FRONT_AHEAD", "PRB_SEED_PAIR_WIDE",
         "PRB_SEED_LOCAL_ORDER", "PRB_SEED_SORT_BITS", "PRB_SEARCH_PAIRS")

# the golden pages need 11 - 14 position bits: only a small PRB_SEED_SORT_BITS leaves bits to the tiles there
LAYOUTS = {
    "default": {},
    "wide": {"PRB_SEED_PAIR_WIDE": "1"},
    "no_local_order": {"PRB_SEED_LOCAL_ORDER": "0"},
    "local_shift0": {"PRB_SEED_SORT_BITS": "4", "PRB_SEED_ROW_SHIFT": "0"},
    "local_shift2": {"PRB_SEED_SORT_BITS": "4", "PRB_SEED_ROW_SHIFT": "2"},
    "local_shift7": {"PRB_SEED_SORT_BITS": "4", "PRB_SEED_ROW_SHIFT": "7"},
}
# chunks smaller than a tile of 2048 pairs, the last one ragged; the front of a sub-batch not issued ahead
VARIANTS = {"whole": {}, "chunks": {"PRB_SEARCH_CHUNK_PAIRS": "300"}, "in_line": {"PRB_NO_FRONT_AHEAD": "1"}}


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def copies(pages):
    return [(np.array(h), np.array(b), tuple(c)) for h, b, c in pages]


@pytest.fixture(scope="module")
def mix(ctx, golden_dir):
    """the 3-page case, all queries in one sub-batch (tiles straddle queries), and its stages 1 - 3 in suffix-array
    order: computed once, never changed"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    db, qb = open_batch(ctx, os.path.join(golden_dir, "mixdb"), seqs)
    mp = pytest.MonkeyPatch()
    set_env(mp, {"PRB_SEED_ROW_SHIFT": "-1"})
    try:
        ref = {stage: copies(capi.search_page(ctx, qb, db, p, capi.default_opts(output_style=1), stage) for p in range(db.npages))
               for stage in (1, 2, 3)}
    finally:
        mp.undo()
    assert sum(r[2][0] for r in ref[3]) > 1000
    yield dict(db=db, qb=qb, ref=ref, nq=len(seqs))
    qb.close()
    db.close()


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_and_tile_order_are_transparent(ctx, mix, monkeypatch, layout, variant):
    from priblast_amd import capi
    db, qb = mix["db"], mix["qb"]
    env = dict(LAYOUTS[layout], **VARIANTS[variant])
    # what the search will choose for these pages: the layouts and the tile order under test are really taken
    for p in range(db.npages):
        lay = capi.seed_pair_layout(db.page_info(p)[1], mix["nq"] - 1, int(env.get("PRB_SEED_ROW_SHIFT", 7)),
                                    int(env.get("PRB_SEED_SORT_BITS", 16)), env.get("PRB_SEED_LOCAL_ORDER") != "0",
                                    env.get("PRB_SEED_PAIR_WIDE") == "1")
        assert lay["narrow"] == (layout != "wide"), (p, lay)
        assert (lay["local_bits"] > 0) == layout.startswith("local_shift"), (p, lay)
    set_env(monkeypatch, env)
    for stage in (1, 2, 3):
        got = [capi.search_page(ctx, qb, db, p, capi.default_opts(output_style=1), stage) for p in range(db.npages)]
        for p, ((h1, b1, c1), (h2, b2, c2)) in enumerate(zip(mix["ref"][stage], got)):
            assert c1 == tuple(c2), (stage, p, c1, c2)
            assert np.array_equal(h1, h2) and np.array_equal(b1, b2), (stage, p)


MASK_FORMS = {
    "narrow": {},
    "narrow_local": {"PRB_SEED_SORT_BITS": "4", "PRB_SEED_ROW_SHIFT": "2"},
    "wide": {"PRB_SEED_PAIR_WIDE": "1"},
    "lists": {"PRB_SEED_FUSED": "0"},
}


@gpu
@pytest.mark.parametrize("chunks", [None, "400"])
@pytest.mark.parametrize("mask", ["every_other_target", "one_query"])
def test_pair_mask_in_both_layouts(ctx, mix, monkeypatch, mask, chunks):
    """the pair mask's test, compaction and sort (A / B buffers swapped behind the compaction) in the narrow layout = the
    wide layout = the list form; `one_query` with small chunks leaves nothing of the other queries' chunks"""
    from priblast_amd import capi
    db, qb = mix["db"], mix["qb"]
    nq, nt = mix["nq"], tbase_of(db)[-1]
    allowed = np.zeros((nq, nt), bool)
    if mask == "one_query":
        allowed[2] = True
    else:
        allowed[:, ::2] = True
    results = {}
    with make_mask(ctx, qb, db, allowed) as m:
        for form, env in MASK_FORMS.items():
            set_env(monkeypatch, dict(env, **({"PRB_SEARCH_CHUNK_PAIRS": chunks} if chunks else {})))
            results[form] = {stage: search(ctx, qb, db, capi.default_opts(output_style=1, allowed_pairs=m.h), stage) for stage in (2, 3)}
    want = results["lists"]
    assert sum(len(h) for h, _, _ in want[3]) > 0
    if mask == "one_query":
        assert all((h["query"] == 2).all() for h, _, _ in want[3])
    for form in ("narrow", "narrow_local", "wide"):
        for stage in (2, 3):
            for p, ((h1, b1, c1), (h2, b2, c2)) in enumerate(zip(want[stage], results[form][stage])):
                assert c1 == c2, (form, stage, p, c1, c2)
                assert np.array_equal(h1, h2) and np.array_equal(b1, b2), (form, stage, p)


# ------------------------------------------------------------------------- the choice of the layout (host only)
def bits_for(v):
    b = 1
    while (1 << b) <= v:
        b += 1
    return b


def layout_restated(nchars, qspan, row_shift, sort_bits, local_order, pair_wide):
    """include/priblast_hip.h, prb_seed_pair_layout"""
    if row_shift < 0:
        return dict(narrow=False, pbits=0, kbits=0, begin=0, local_bits=0, wide_key=False)
    qbits, pbits = bits_for(max(1, qspan)), bits_for(max(1, nchars - 1))
    if not pair_wide and pbits + qbits <= 32:
        shift = min(row_shift, pbits)
        g = min(max(shift, pbits + qbits - sort_bits), shift + 5) if local_order else shift
        return dict(narrow=True, pbits=pbits, kbits=pbits + qbits, begin=g, local_bits=g - shift, wide_key=False)
    pbits = bits_for(max(1, (nchars - 1) >> row_shift))
    return dict(narrow=False, pbits=pbits, kbits=pbits + qbits, begin=0, local_bits=0, wide_key=pbits + qbits > 32)


def L(narrow, pbits, kbits, begin, local_bits, wide_key=False):
    return dict(narrow=narrow, pbits=pbits, kbits=kbits, begin=begin, local_bits=local_bits, wide_key=wide_key)


EDGES = [
    # (nchars, query span, row_shift, sort_bits, local_order, pair_wide) -> layout
    ((2 ** 27, 31, 7, 16, True, False), L(True, 27, 32, 12, 5)),        # 27 + 5 = 32 bits exactly; g = 16 capped at 7 + 5
    ((2 ** 27, 32, 7, 16, True, False), L(False, 20, 26, 0, 0)),        # 27 + 6 = 33 bits: wide, key (query, position >> 7)
    ((2 ** 27 + 1, 31, 7, 16, True, False), L(False, 21, 26, 0, 0)),    # 28 + 5 = 33 bits
    ((2 ** 27, 0, 7, 16, True, False), L(True, 27, 28, 12, 5)),         # one query of the benchmark's page: 28 - 16 = 12
    ((2 ** 27, 0, 7, 20, True, False), L(True, 27, 28, 8, 1)),
    ((2 ** 27, 0, 7, 21, True, False), L(True, 27, 28, 7, 0)),          # the sort covers everything above the row shift
    ((2 ** 27, 0, 7, 32, True, False), L(True, 27, 28, 7, 0)),
    ((2 ** 27, 0, 7, 16, False, False), L(True, 27, 28, 7, 0)),         # PRB_SEED_LOCAL_ORDER=0
    ((2 ** 27, 0, 0, 16, True, False), L(True, 27, 28, 5, 5)),          # g = 12 capped at 0 + 5
    ((2 ** 27, 0, 14, 16, True, False), L(True, 27, 28, 14, 0)),        # the row shift is above 28 - 16 already
    ((2 ** 27, 0, 30, 16, True, False), L(True, 27, 28, 27, 0)),        # a row shift beyond the position bits: by query alone
    ((2 ** 27, 0, 7, 16, True, True), L(False, 20, 21, 0, 0)),          # PRB_SEED_PAIR_WIDE=1
    ((2 ** 27, 0, -1, 16, True, False), L(False, 0, 0, 0, 0)),          # suffix-array order: no pair sort
    ((2 ** 27, 0, -1, 16, True, True), L(False, 0, 0, 0, 0)),
    ((2 ** 24, 0, 7, 16, True, False), L(True, 24, 25, 9, 2)),          # 25 - 16 = 9: two bits left to the tiles
    ((2 ** 20, 0, 7, 16, True, False), L(True, 20, 21, 7, 0)),          # 21 - 16 = 5 < 7
    ((5000, 7, 0, 4, True, False), L(True, 13, 16, 5, 5)),              # the sizes of the golden pages
    ((5000, 7, 2, 4, True, False), L(True, 13, 16, 7, 5)),
    ((5000, 7, 7, 4, True, False), L(True, 13, 16, 12, 5)),
    ((2 ** 31 - 1, 1000, 0, 16, True, False), L(False, 31, 41, 0, 0, True)),  # 64-bit keys
    ((1, 0, 7, 16, True, False), L(True, 1, 2, 1, 0)),
]


@pytest.mark.parametrize("args,want", EDGES)
def test_layout_choice_at_the_edges(args, want):
    from priblast_amd import capi
    assert capi.seed_pair_layout(*args) == want
    assert layout_restated(*args) == want


def test_layout_choice_equals_the_restatement():
    from priblast_amd import capi
    rng = np.random.default_rng(3)
    for _ in range(2000):
        args = (int(2 ** rng.uniform(0, 31)), int(2 ** rng.uniform(0, 12)) - 1, int(rng.integers(-1, 31)), int(rng.integers(1, 33)),
                bool(rng.integers(2)), bool(rng.integers(8) == 0))
        got = capi.seed_pair_layout(*args)
        assert got == layout_restated(*args), args
        if got["narrow"]:
            assert got["kbits"] <= 32 and 0 <= got["local_bits"] <= 5 and got["begin"] < got["kbits"]
            assert got["begin"] - got["local_bits"] == min(args[2], got["pbits"])
