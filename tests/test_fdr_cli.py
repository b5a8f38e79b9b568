"""`ris -t -z 6 -Z 1 -Q` on the golden mix database: the lines with the three columns stripped are byte for byte the lines
of the same command without -Q, and the three columns are tests/fdr_ref.py's figures from the Decoys and NullLE columns of
that run with the query's number of targets - plain, with -H 1 -D 2, with -u, under the pair list of test_null_cli.py
(Tests = the targets listed for the query), and with PRB_BATCH=1.  The unmasked runs of the golden data have 5 lines of 28
with QValue < 1, the run under the list 3 of 4: every test prints its count and asserts that there are some."""
import os
import subprocess

import pytest

import fdr_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
LISTED = [("mq0", "mdb14"), ("mq1", "mdb3"), ("mq1", "mdb14"), ("mq_rc", "mdb0"), ("mq3", "mdb20")]
EVERY = ["mdb7"]
BASE = ["-t", "-z", "6", "-Z", "1"]
TAIL = ", Tests, Rank, Q Value"


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def run(tmp_path, db, extra, out, **env):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / out), "-d", db] + BASE + extra, capture_output=True,
                       text=True, env=clean_env(**env))
    assert r.returncode == 0, r.stderr
    with open(tmp_path / out) as f:
        return f.read().split("\n")


def check(plain, with_q, tests_of):
    """-> the lines with QValue < 1.  tests_of(query name) = the query's hypotheses"""
    assert len(plain) == len(with_q) and plain[:2] == with_q[:2]
    assert with_q[2] == plain[2] + TAIL and plain[2].endswith("P Value") and plain[-1] == with_q[-1] == ""
    body, body_q = plain[3:-1], with_q[3:-1]
    assert [l.rsplit(",", 3)[0] for l in body_q] == body  # the parent's lines, byte for byte
    pairs, tests = [], {}
    for l in body:
        qname = l.split(",")[1]
        decoys, _, null_le = l.rsplit(",", 5)[1:4]
        pairs.append((qname, int(null_le), int(decoys)))
        tests[qname] = tests_of(qname)
    figs = fdr_ref.fdr(pairs, tests)
    for l, fig in zip(body_q, figs):
        assert ",".join(l.rsplit(",", 3)[1:]) == fdr_ref.columns(fig), l
    return sum(1 for f in figs if f[2:] != (0, 0, 0) and fdr_ref.q_value(f[0], *f[2:]) < 1), len(body)


CASES = {"plain": [], "seq": ["-H", "1", "-D", "2"], "distinct": ["-u"]}


@pytest.mark.parametrize("tag", list(CASES))
def test_columns_equal_the_reference(tmp_path, golden_dir, tag):
    """5 of the 28 lines of each of these runs have QValue < 1 (measured on the parent's output through fdr_ref)"""
    db = os.path.join(golden_dir, "mixdb")
    ntargets = len(refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))[0])
    extra = CASES[tag]
    plain, with_q = run(tmp_path, db, extra, tag), run(tmp_path, db, extra + ["-Q"], tag + "_q")
    below, lines = check(plain, with_q, lambda q: ntargets)
    print(f"{tag}: lines with QValue < 1: {below} of {lines}")
    assert lines > 10 and below > 0
    if tag == "plain":  # single-query batches: the same bytes
        assert run(tmp_path, db, extra + ["-Q"], tag + "_b1", PRB_BATCH="1") == with_q


def test_under_a_pair_list(tmp_path, golden_dir):
    """Tests = the targets listed for the query (1 to 3 here); 3 of the 4 lines have QValue < 1"""
    db = os.path.join(golden_dir, "mixdb")
    dbnames = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))[0]
    (tmp_path / "pairs.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in LISTED) + "".join(f"*\t{t}\n" for t in EVERY))
    listed = lambda q: sum(1 for n in dbnames if n in EVERY or (q, n) in LISTED)
    extra = ["-L", str(tmp_path / "pairs.tsv")]
    plain, with_q = run(tmp_path, db, extra, "listed"), run(tmp_path, db, extra + ["-Q"], "listed_q")
    below, lines = check(plain, with_q, listed)
    print(f"listed: lines with QValue < 1: {below} of {lines}")
    assert lines > 0 and below > 0
    assert {int(l.rsplit(",", 3)[1]) for l in with_q[3:-1]} <= {1, 2, 3}
    assert run(tmp_path, db, extra + ["-Q"], "listed_b1", PRB_BATCH="1") == with_q
