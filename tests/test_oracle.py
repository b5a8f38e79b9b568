"""Pins the CPU oracle (oracle/*.c) against golden vectors produced by the UNMODIFIED, compiled
reference (strict build; tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest

import refdump

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_fmath_tables_and_probes(oracle):
    L = oracle.lib()
    t = refdump.read_tables(os.path.join(GOLDEN, "tables.bin"))
    et = np.ctypeslib.as_array(L.orc_expd_table(), (2048,))
    lt = np.ctypeslib.as_array(L.orc_log_table(), (4096,))
    assert np.array_equal(et, t["expd_tbl"])
    assert np.array_equal(bits32(lt), bits32(t["log_tbl"]))
    for x, y in t["expd_probe"]:
        assert bits64(L.orc_expd(float(x))) == bits64(y), x
    for x, y in t["log_probe"]:
        assert bits32(L.orc_logf(float(x))) == bits32(y), x
    # the two edge values the accessibility code relies on
    assert abs(L.orc_logf(float("inf")) - 88.722839) < 1e-5
    assert abs(L.orc_logf(0.0) + 88.029694) < 1e-4
    assert L.orc_expd(-708.4) == 0.0


WIDE = [("widew.fa", f"widew_w{W}d{d}.racc") for W, d in ((100, 5), (129, 5), (129, 2), (150, 5), (200, 4))]
# the spans the HIP kernels change form at (64 / 65 cells per pass, 96 / 97 for the row masks, 127 / 128 for the two-pass
# mapping) and the limit 255, the last on the sequences of at most 700 nt
WIDE += [("widew.fa", f"widew_w{W}d5.racc") for W in (64, 65, 96, 97, 128)] + [("widew_short.fa", "widew_w255d2.racc")]


@pytest.mark.parametrize("fa,racc", [("corpus.fa", "corpus.racc"), ("c1_q.fa", "c1_q_w40d7.racc")] + WIDE)
def test_raccess_bit_exact(oracle, fa, racc):
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, fa))
    g = refdump.read_raccess(os.path.join(GOLDEN, racc))
    assert len(seqs) == len(g["seqs"])
    for name, s, rec in zip(names, seqs, g["seqs"]):
        acc, cond = oracle.raccess(s, g["W"], g["delta"])
        assert np.array_equal(bits32(acc), bits32(rec["acc"])), name
        assert np.array_equal(bits32(cond), bits32(rec["cond"])), name


def test_corpus_exercises_both_biloop_branches(oracle):
    """gc2000/len2700 must sit in the log-sum branch (|logZ| > 690), len1000 in the overflow regime."""
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "corpus.fa"))
    d = dict(zip(names, seqs))
    _, _, t = oracle.raccess(d["len1000"], 70, 5, debug=True)
    assert 89 < t["alpha_outer"][-1] < 690
    _, _, t = oracle.raccess(d["len2700"], 70, 5, debug=True)
    assert t["alpha_outer"][-1] > 690
    _, _, t = oracle.raccess(d["len330"], 70, 5, debug=True)
    assert t["alpha_outer"][-1] < 95


def test_encoder_and_suffix_array(oracle):
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "c1_q.fa"))
    g = refdump.read_sa(os.path.join(GOLDEN, "c1_q.sa"))
    for s, (enc, sa) in zip(seqs, g):
        e2, sa2 = oracle.encode_and_sa(s)
        assert np.array_equal(e2, enc)
        assert np.array_equal(sa2, sa)


def test_db_suffix_array_matches_reference_ind(oracle, golden_dir):
    """The oracle's suffix-array builder reproduces the SA the reference stored in .ind."""
    seq = np.fromfile(os.path.join(golden_dir, "c1db.seq"), dtype=np.uint8)
    nseq = int(np.frombuffer(seq[:4].tobytes(), "<i4")[0])
    off = 4 + 4 * nseq
    nchars = int(np.frombuffer(seq[off:off + 4].tobytes(), "<i4")[0])
    T = seq[off + 4:off + 4 + nchars].copy()
    ind = np.fromfile(os.path.join(golden_dir, "c1db.ind"), dtype="<i4")
    assert ind[0] == nchars
    sa = np.zeros(nchars, np.int32)
    oracle.lib().orc_suffix_array(T.ctypes.data, sa.ctypes.data, nchars)
    assert np.array_equal(sa, ind[1:1 + nchars])


def _key(h):
    return (h["db_sp"], h["q_sp"], -h["db_len"], -h["q_len"], h["e_tot"],
            h["db_id"], h["db_id_start"], tuple(map(tuple, h["bp"])))


def _same_hit(a, b, split_tol=0.0):
    """Exact on coordinates and on the total energy.  `split_tol` > 0 relaxes only the
    acc/hyb split: after the ungapped stage two different seeds can extend to the same
    region with bit-identical total energy but hybridization sums that differ in the last
    bit (sums of 0.01 multiples in a different order); which of the two survives the
    redundancy filter depends on the reference's unspecified std::sort tie order.  (After
    the gapped stage the comparison is exact; twins that survive it with different base
    pairs are excused only on proof, tests/tiecheck.py and DESIGN.md 2, deviation 1.)"""
    for k in ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start"):
        if a[k] != b[k]:
            return False
    if bits64(a["e_tot"]) != bits64(b["e_tot"]):
        return False
    for k in ("e_acc", "e_hyb"):
        if split_tol == 0.0 and bits64(a[k]) != bits64(b[k]):
            return False
        if abs(a[k] - b[k]) > split_tol:
            return False
    return np.array_equal(a["bp"], b["bp"])


@pytest.mark.parametrize("tag", ["c1", "mix", "quirk"])
def test_stage_dumps(oracle, golden_dir, tag):
    """Per-stage parity: seed hits in the reference's emission order; post-extension lists as
    multisets (the reference's std::sort leaves ties of its comparator unordered)."""
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
    stg = refdump.read_stages(os.path.join(golden_dir, f"{tag}.stg"))
    db = oracle.Db(os.path.join(golden_dir, f"{tag}db"))
    nseed = nung = ngap = 0
    try:
        for rec in stg:
            seed, ung, gap = db.stages(seqs[rec["q"]], rec["page"])
            assert len(seed) == len(rec["seed"])
            for a, b in zip(seed, rec["seed"]):
                assert _same_hit(a, b)
            for mine, ref, tol in ((ung, rec["ungapped"], 1e-12), (gap, rec["gapped"], 0.0)):
                assert len(mine) == len(ref)
                for a, b in zip(sorted(mine, key=_key), sorted(ref, key=_key)):
                    assert _same_hit(a, b, tol)
            nseed += len(seed)
            nung += len(ung)
            ngap += len(gap)
    finally:
        db.close()
    assert nseed > 0 and nung > 0 and ngap > 0
    if tag == "c1":
        assert (nseed, nung, ngap) == (42110, 6352, 127)


@pytest.mark.parametrize("tag", ["c1", "mix", "quirk"])
@pytest.mark.parametrize("style", [0, 1])
def test_ris_output_matches_reference(oracle, golden_dir, tmp_path, tag, style):
    out = str(tmp_path / "o.out")
    n = oracle.ris(os.path.join(GOLDEN, f"{tag}_q.fa"), os.path.join(golden_dir, f"{tag}db"), out,
                   nthreads=4, output_style=style)
    with open(os.path.join(GOLDEN, f"{tag}_ris_s{style}.out")) as f:
        gold = f.read().splitlines()
    with open(out) as f:
        head = f.read().splitlines()[:3]
    assert head[0] == gold[0] and head[2] == gold[1]
    body = oracle.sorted_body(out)
    assert n == len(body) == len(gold) - 2
    assert body == gold[2:]


def test_quirk_fixture_holds_unsorted_final_hits(oracle, golden_dir):
    """The point of the `quirk` case (rna_interaction_search.cpp:314-317): final hits of the
    REFERENCE whose stored base pairs are not ascending - hit 0 of a (query, page) list keeps
    [diagonal, left chain, right chain outer->inner] - with a left and a right extension among them, and the
    restatement reproduces each of them pair for pair (test_stage_dumps compares the lists in order)."""
    stg = refdump.read_stages(os.path.join(golden_dir, "quirk.stg"))
    shapes = set()
    for rec in stg:
        for h in rec["gapped"]:
            q = [int(p[0]) for p in h["bp"]]
            if q != sorted(q):
                shapes.add("right" if q[-1] < max(q) and q[0] == min(q) else "left")
    assert shapes == {"left", "right"}
    with open(os.path.join(GOLDEN, "quirk_ris_s1.out")) as f:
        body = f.read().splitlines()[2:]
    unsorted_lines = 0
    for line in body:
        q = [int(t[1:].split(":")[0]) for t in line.split(",")[-1].split()]
        unsorted_lines += q != sorted(q)
    assert unsorted_lines >= 4
