"""`ris -k K -E M [-Z SEED]` on the GPU: with the five columns cut off the output is that of `ris -k K`, byte for byte,
and the columns are those of tests/eval_ref.py over PLAIN runs of `ris`: of the queries, and of a FASTA file of their
decoys written here through capi.shuffle_sequence (a decoy is shuffled with its query's place in the input file).  The
plain runs write binary records (-b), so the energies compared are the doubles, not their six printed digits."""
import os
import struct
import subprocess

import numpy as np
import pytest

import eval_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
K, M, SEED = 5, 3, 1
LISTED = [("mq0", "mdb14"), ("mq1", "mdb3"), ("mq1", "mdb14"), ("mq_rc", "mdb0"), ("mq3", "mdb20")]
EVERY = ["mdb7"]


def ris(tmp_path, db, extra, out, queries=QUERIES, **env):
    from priblast_amd import capi
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", queries, "-o", str(tmp_path / out), "-d", db] + extra, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr
    return tmp_path / out


def read_hits(path):
    """a binary hit file (`ris -b`) -> [(query name, e_tot)] in output order"""
    from priblast_amd import capi
    blob = open(path, "rb").read()
    at = [0]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, blob, at[0])
        at[0] += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def text():
        n = take("i")
        at[0] += n
        return blob[at[0] - n:at[0]].decode()

    assert blob[:8] == b"PRBHITS\x01"
    at[0] = 8
    _, npages = take("ii")
    text()
    for _ in range(npages):
        for _ in range(take("i")):
            take("iii")
            text()
    out = []
    while True:
        tag = take("q")
        if tag == ord("E"):
            assert take("q") == len(out)
            return out
        assert tag == ord("B")
        names = []
        for _ in range(take("q")):
            names.append(text())
            take("i")
        pages = []
        for _ in range(npages):
            nh, npairs = take("qq")
            pages.append(np.frombuffer(blob, capi.HIT_DTYPE, nh, at[0]))
            at[0] += nh * capi.HIT_DTYPE.itemsize + npairs * 8
        for q in range(len(names)):  # (the text's order: query by query, page by page)
            for h in pages:
                out += [(names[q], float(e)) for e in h["e_tot"][h["query"] == q]]


def expected_columns(tmp_path, db, extra, tag, pairs=None):
    """the column text per `-k K` line, in the lines' order, from plain runs with the switches `extra`"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(QUERIES)
    assert len(set(names)) == len(names)
    with open(tmp_path / f"{tag}_decoys.fa", "w") as f:
        for i, (n, s) in enumerate(zip(names, seqs)):
            for d in range(M):
                f.write(f">{n}~{d}\n{capi.shuffle_sequence(s, SEED, i, d)}\n")
    dextra = list(extra)
    if pairs is not None:
        (tmp_path / f"{tag}_dpairs.tsv").write_text("".join(f"{q}~{d}\t{t}\n" for q, t in LISTED for d in range(M)) + "".join(f"*\t{t}\n" for t in EVERY))
        dextra += ["-L", str(tmp_path / f"{tag}_dpairs.tsv")]
        extra = list(extra) + ["-L", str(pairs)]
    real = read_hits(ris(tmp_path, db, ["-b"] + list(extra), f"{tag}_real.bin"))
    dec = read_hits(ris(tmp_path, db, ["-b"] + dextra, f"{tag}_dec.bin", queries=str(tmp_path / f"{tag}_decoys.fa")))
    idx = {n: i for i, n in enumerate(names)}
    rq, re_ = np.array([idx[n] for n, _ in real]), np.array([e for _, e in real])
    dq, de = np.array([idx[n.rsplit("~", 1)[0]] for n, _ in dec], np.int64), np.array([e for _, e in dec])
    # the K best of every query, best first, ties in output order; the queries in the output's order (longest first, stable)
    lq, le = [], []
    for q in sorted(range(len(seqs)), key=lambda i: -len(seqs[i])):
        mine = re_[rq == q]
        for e in mine[np.argsort(mine + 0.0, kind="stable")[:K]]:
            lq.append(q), le.append(e)
    want = eval_ref.score(len(names), rq, re_, dq, de, M, look_q=lq, look_e=le)
    return want, [",%d,%d,%d,%s,%s" % (r["decoys"], r["null_le"], r["rank"], "%g" % eval_ref.evalue(r), "%g" % eval_ref.qvalue(r)) for r in want]


def check(tmp_path, db, extra, tag, pairs=None):
    cli = list(extra) + (["-L", str(pairs)] if pairs is not None else [])
    plain = open(ris(tmp_path, db, ["-k", str(K)] + cli, f"{tag}_k")).read().split("\n")
    scored_path = ris(tmp_path, db, ["-k", str(K), "-E", str(M), "-Z", str(SEED)] + cli, f"{tag}_ke")
    scored = open(scored_path).read().split("\n")
    assert len(plain) == len(scored) and plain[:2] == scored[:2] and plain[-1] == scored[-1] == ""
    assert scored[2] == plain[2] + ", Decoys, Null LE, Rank, E Value, Q Value"
    recs, want = expected_columns(tmp_path, db, extra, tag, pairs)
    assert len(want) == len(plain) - 4 > 0
    for line, base, cols in zip(scored[3:-1], plain[3:-1], want):
        assert line.rsplit(",", 5)[0] == base, line
        assert line[len(base):] == cols, (line, cols)
    return scored_path, recs


def test_columns_equal_the_reference_and_the_lines_are_those_of_k(tmp_path, golden_dir):
    db = os.path.join(golden_dir, "mixdb")
    out, want = check(tmp_path, db, [], "all")
    assert (want["null_le"] > 0).any() and (want["null_le"] == 0).any() and (eval_ref.qvalue(want) < 1).any()  # (not vacuous)
    # one query per batch gives the same bytes: a query's figures do not depend on its batch
    assert ris(tmp_path, db, ["-k", str(K), "-E", str(M), "-Z", str(SEED)], "b1", PRB_BATCH="1").read_bytes() == out.read_bytes()


def test_with_distinct_sites(tmp_path, golden_dir):
    check(tmp_path, os.path.join(golden_dir, "mixdb"), ["-u"], "u")


def test_with_the_detailed_style_and_looser_thresholds(tmp_path, golden_dir):
    check(tmp_path, os.path.join(golden_dir, "mixdb"), ["-s", "1", "-f", "-3", "-g", "-6.5"], "s1")


def test_under_a_pair_list_a_decoy_is_searched_against_its_owners_listed_targets(tmp_path, golden_dir):
    db = os.path.join(golden_dir, "mixdb")
    (tmp_path / "pairs.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in LISTED) + "".join(f"*\t{t}\n" for t in EVERY))
    check(tmp_path, db, [], "listed", pairs=tmp_path / "pairs.tsv")
