"""The `edge` golden case (tests/golden/make_golden.py: edge_inputs): the DATABASE side at its edges - targets of 4 to
33 nt next to each other, targets that are nothing but a site, trap neighbours behind the separators, sites at text
position 0 and nchars - 1, a page of one sequence.  CPU only: the conditions the fixture must keep meeting when it is
regenerated, and the restatement (oracle/*.c) against what the unmodified reference produced for it."""
import os

import numpy as np
import pytest

import refdump
from test_oracle import _key, _same_hit, bits32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAPS = ("ed_trap1", "ed_trap2")   # site-only targets between two trap neighbours
NHASH = sum(4 ** (i + 1) for i in range(8))


@pytest.fixture(scope="module")
def edge_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge")
    refdump.unpack_case(GOLDEN, "edge", str(d))
    return str(d)


def final_hits(edge_dir):
    """Every final hit of the reference with its sequence's text interval: dicts with page, q, id, s (text position of
    the sequence's first character), L, lo, hi (the hit's text interval), bp."""
    pages = refdump.read_seq_pages(os.path.join(edge_dir, "edgedb.seq"))
    out = []
    for rec in refdump.read_stages(os.path.join(edge_dir, "edge.stg")):
        pg = pages[rec["page"]]
        for h in rec["gapped"]:
            i = h["db_id"]
            out.append({"page": rec["page"], "q": rec["q"], "id": i, "s": int(pg["start"][i]), "L": int(pg["len"][i]),
                        "lo": h["db_sp"], "hi": h["db_sp"] + h["db_len"] - 1, "bp": h["bp"], "nseq": len(pg["len"])})
    return pages, out


def gapped(h):
    return len(set((h["bp"][:, 0] - h["bp"][:, 1]).tolist())) > 1


def test_edge_fixture_conditions(edge_dir):
    pages, hits = final_hits(edge_dir)
    names, _ = refdump.read_fasta(os.path.join(GOLDEN, "edge_db.fa"))
    first_id = np.concatenate([[0], np.cumsum([len(p["len"]) for p in pages])])
    # the layout: at least 3 pages, the last of one sequence, a target of every tiny length
    assert len(pages) >= 3 and len(pages[-1]["len"]) == 1
    assert {4, 5, 7, 8, 9, 20, 31, 32, 33} <= set(np.concatenate([p["len"] for p in pages]).tolist())
    for h in hits:  # no hit leaves its sequence
        assert h["s"] <= h["lo"] <= h["hi"] <= h["s"] + h["L"] - 1, h
    at_end = [h for h in hits if h["lo"] == h["s"] or h["hi"] == h["s"] + h["L"] - 1]
    assert len(at_end) >= 6
    assert any(h["id"] == 0 for h in at_end) and any(h["id"] == h["nseq"] - 1 for h in at_end)
    assert any(h["lo"] == 0 for h in at_end)                                         # text position 0
    assert any(h["hi"] == len(pages[h["page"]]["text"]) - 2 for h in at_end)         # the base before the last 0
    assert sum(gapped(h) for h in at_end) >= 2
    assert any(h["lo"] == h["s"] and h["hi"] == h["s"] + h["L"] - 1 for h in hits)
    for t in TRAPS:
        g = names.index(t)
        mine = [h for h in hits if first_id[h["page"]] + h["id"] == g]
        assert mine, t
        assert all(h["hi"] - h["lo"] + 1 <= len_of(pages, first_id, g) for h in mine), t
        # and its two neighbours are tiny and on the same page
        page = int(np.searchsorted(first_id, g, side="right")) - 1
        assert first_id[page] < g < first_id[page + 1] - 1
        assert len_of(pages, first_id, g - 1) <= 9 and len_of(pages, first_id, g + 1) <= 9
    assert set(range(len(pages))) - {h["page"] for h in hits}                        # a page without hits
    assert max(np.bincount(p["start"] // 32).max() for p in pages) >= 5              # starts per 32-character block


def len_of(pages, first_id, g):
    page = int(np.searchsorted(first_id, g, side="right")) - 1
    return int(pages[page]["len"][g - first_id[page]])


def test_edge_stage_dumps(oracle, edge_dir):
    """test_oracle.py::test_stage_dumps on the edge case."""
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_q.fa"))
    stg = refdump.read_stages(os.path.join(edge_dir, "edge.stg"))
    db = oracle.Db(os.path.join(edge_dir, "edgedb"))
    n = [0, 0, 0]
    try:
        for rec in stg:
            where = (names[rec["q"]], rec["page"])
            seed, ung, gap = db.stages(seqs[rec["q"]], rec["page"])
            assert len(seed) == len(rec["seed"]), where
            for a, b in zip(seed, rec["seed"]):
                assert _same_hit(a, b), (where, a, b)
            for mine, ref, tol in ((ung, rec["ungapped"], 1e-12), (gap, rec["gapped"], 0.0)):
                assert len(mine) == len(ref), where
                for a, b in zip(sorted(mine, key=_key), sorted(ref, key=_key)):
                    assert _same_hit(a, b, tol), (where, a, b)
            for k, l in enumerate((seed, ung, gap)):
                n[k] += len(l)
    finally:
        db.close()
    assert min(n) > 0


@pytest.mark.parametrize("style", [0, 1])
def test_edge_ris_output(oracle, edge_dir, tmp_path, style):
    out = str(tmp_path / "o.out")
    n = oracle.ris(os.path.join(GOLDEN, "edge_q.fa"), os.path.join(edge_dir, "edgedb"), out, nthreads=4, output_style=style)
    with open(os.path.join(GOLDEN, f"edge_ris_s{style}.out")) as f:
        gold = f.read().splitlines()
    with open(out) as f:
        head = f.read().splitlines()[:3]
    assert head[0] == gold[0] and head[2] == gold[1]
    body = oracle.sorted_body(out)
    assert n == len(body) == len(gold) - 2
    assert body == gold[2:]


def test_edge_suffix_arrays(oracle, edge_dir):
    """orc_suffix_array of every page's text against .ind: the 40-character page of 4-nt targets and the page of one
    sequence included."""
    pages = refdump.read_seq_pages(os.path.join(edge_dir, "edgedb.seq"))
    ind = np.fromfile(os.path.join(edge_dir, "edgedb.ind"), dtype="<i4")
    at = 0
    for p, pg in enumerate(pages):
        n = len(pg["text"])
        assert ind[at] == n, p
        sa = np.zeros(n, np.int32)
        text = np.ascontiguousarray(pg["text"])
        oracle.lib().orc_suffix_array(text.ctypes.data, sa.ctypes.data, n)
        assert np.array_equal(sa, ind[at + 1:at + 1 + n]), p
        at += 1 + n + 2 * NHASH
    assert at == len(ind)


def test_edge_accessibilities(oracle, edge_dir):
    """oracle.raccess of every target against .acc, bit for bit: L - 4 accessibilities (none for a 4-nt target) and L
    conditional ones."""
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "edge_db.fa"))
    bas = np.fromfile(os.path.join(edge_dir, "edgedb.bas"), dtype="<i4")
    W, delta = int(bas[2]), int(bas[3])
    recs = refdump.read_acc(os.path.join(edge_dir, "edgedb.acc"), len(seqs))
    for name, s, (n, acc, m, cond) in zip(names, seqs, recs):
        assert (n, m) == (len(s) - delta + 1, len(s)), name
        oacc, ocond = oracle.raccess(s, W, delta)
        assert np.array_equal(bits32(oacc[:n]), bits32(acc)), name
        assert np.array_equal(bits32(ocond), bits32(cond)), name
