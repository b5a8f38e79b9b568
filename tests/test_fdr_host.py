"""`ris -t -z N -Q` without a GPU: tests/fdr_ref.py against a brute-force restatement of the definition, the 41-bit sort
key of a p-value against exact rationals, the host line writer on hand-made records (through tests/fdr_lines_check.cpp, a
stand-alone program), the usage text and the refusals - made before any GPU work."""
import os
import random
import subprocess
from fractions import Fraction

import pytest

import fdr_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QUERIES = os.path.join(HERE, "golden", "mix_q.fa")

Z = "-z (an empirical p-value per pair from N shuffled decoys)"
Q = "-Q (a Benjamini-Hochberg q-value per pair of the null table)"
REFUSALS = {
    "-t -Q": f"Error: {Q} needs {Z}",
    "-Q": f"Error: {Q} needs {Z}",
    "-t -G groups.tsv -P 3 -Q": f"Error: {Q} needs {Z}",
    "-t -A annot.tsv -F 3 -Q": f"Error: {Q} needs {Z}",
    "-k 2 -E 3 -Q": f"Error: {Q} needs {Z}",
    "-t -z 4 -Q -n 2": f"Error: {Z} can't be combined with -n (the N best pairs per query)",
    "-z 4 -Q -r 2": f"Error: {Z} can't be combined with -r (the N best queries per target)",
    "-z 4 -Q -c 2": f"Error: {Z} can't be combined with -c (the regions of each target bound by at least D queries)",
}


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.mark.parametrize("extra", list(REFUSALS))
def test_refused_before_any_gpu_work(tmp_path, extra):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", str(tmp_path / "nodb")] + extra.split(),
                       capture_output=True, text=True, env=clean_env())
    assert (r.stderr.splitlines() or [""])[0] == REFUSALS[extra]
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_q_takes_no_argument(tmp_path):
    """`-Q -z 4`: were -Q to take an argument it would swallow -z, and the refusal would be -Q's need of -z"""
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", str(tmp_path / "nodb"), "-Q", "-z", "4"],
                       capture_output=True, text=True, env=clean_env())
    assert (r.stderr.splitlines() or [""])[0] == f"Error: {Z} needs -t (per-pair summary lines)"


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "    -Q        with -t -z N" in text and "Benjamini-Hochberg" in text and "QValue" in text


# ------------------------------------------------------------------------- the reference against the definition
@pytest.mark.parametrize("seed", range(12))
def test_ref_equals_the_brute_force_restatement(seed):
    rng = random.Random(seed)
    n = rng.randrange(0, 40)
    top = rng.choice([3, 6, 12])  # small denominators: many equal and many tied p-values
    pairs = []
    for _ in range(n):
        d = rng.randrange(1, top + 1)
        pairs.append((rng.randrange(3), rng.randrange(0, d + 1), d))
    count = {q: sum(1 for p in pairs if p[0] == q) for q in range(3)}
    for tests in ({q: max(1, count[q]) for q in range(3)}, {q: count[q] + 1 + 3 * q for q in range(3)}, {q: 2 ** 31 - 1 for q in range(3)}):
        got = fdr_ref.fdr(pairs, tests)
        assert got == fdr_ref.brute(pairs, tests)
        for (q, le, d), (t, rank, qn, qd, qr) in zip(pairs, got):
            assert t == tests[q] and 1 <= rank <= count[q]
            assert (qn, qd, qr) == (0, 0, 0) or (Fraction(t * qn, qd * qr) <= 1 and Fraction(t * qn, qd * qr) <= Fraction(t * (le + 1), (d + 1) * rank))


def test_ref_on_a_hand_made_query():
    """5 pairs, 10 tests: p = 1/11, 1/11, 2/4 = 1/2 twice (different denominators), 1"""
    pairs = [(0, 0, 10), (0, 1, 3), (0, 10, 10), (0, 0, 10), (0, 0, 1)]
    got = fdr_ref.fdr(pairs, {0: 10})
    # ranks: 1/11 -> 2, 1/2 -> 4, 1 -> 5.  FDR: 10/(11*2) = 5/11; 10*2/(4*4) = 10*1/(2*4) = 5/4; 10*11/(11*5) = 2
    assert [g[1] for g in got] == [2, 4, 5, 2, 4]
    assert got[0] == got[3] == (10, 2, 1, 11, 2)
    assert got[1] == (10, 4, 0, 0, 0) and got[4] == (10, 4, 0, 0, 0) and got[2] == (10, 5, 0, 0, 0)
    assert fdr_ref.columns(got[0]) == "10,2,0.454545" and fdr_ref.columns(got[2]) == "10,5,1"
    # with 4 tests the tie of 1/2 and 2/4 decides a triple: FDR = 4*1/(2*4) = 1/2 for both, the lower den wins
    got = fdr_ref.fdr(pairs, {0: 5})
    assert got[1] == got[4] == (5, 4, 1, 2, 4) and fdr_ref.columns(got[1]) == "5,4,0.625"


# ------------------------------------------------------------------------- the sort key
def assert_key_orders(fracs):
    fracs = sorted(fracs, key=lambda f: Fraction(*f))
    for (an, ad), (bn, bd) in zip(fracs, fracs[1:]):
        ka, kb = fdr_ref.p_key(an, ad), fdr_ref.p_key(bn, bd)
        assert 0 <= ka <= kb <= 1 << 40
        assert (ka == kb) == (Fraction(an, ad) == Fraction(bn, bd)), (an, ad, bn, bd)


def test_key_orders_small_denominators_exactly():
    assert_key_orders([(n, d) for d in range(1, 61) for n in range(1, d + 1)])


def test_key_orders_the_largest_denominators():
    """two distinct fractions with denominators <= 100001 differ by 1 / (100001 * 100000) > 2^-40 at least: the closest
    pairs are n / 100001 against n / 100000 and their neighbours"""
    rng = random.Random(5)
    fracs = []
    for d in (100001, 100000, 99999, 99991, 50001, 50000):
        fracs += [(n, d) for n in (1, 2, 3, d - 2, d - 1, d)]
        fracs += [(rng.randrange(1, d + 1), d) for _ in range(300)]
    for n in [1, 2, 49999, 50000, 50001, 99998, 99999, 100000] + [rng.randrange(1, 100001) for _ in range(300)]:
        fracs += [(n, 100001), (n, 100000), (n + 1, 100001), (max(1, n - 1), 100000)]
    assert_key_orders(fracs)
    assert 2 ** 40 < 100001 * 100000 * 2 ** 7  # (the margin is not large: 2^-40 against 2^-33.2)


# ------------------------------------------------------------------------- the line writer
@pytest.fixture(scope="module")
def lines_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fdr_lines") / "fdr_lines_check")
    host = os.path.join(ROOT, "priblast_amd", "host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fopenmp", "-ffp-contract=off", "-I", host, "-o", exe, os.path.join(HERE, "fdr_lines_check.cpp"),
                    os.path.join(host, "output.cpp"), os.path.join(host, "cpu_budget.cpp")], check=True)
    return exe


def test_line_writer_appends_the_three_columns(lines_check):
    pairs = [(0, 0, 10), (0, 1, 3), (0, 10, 10), (0, 0, 10), (2, 0, 1), (2, 3, 99999)]
    figs = fdr_ref.fdr(pairs, {0: 10, 2: 2 ** 31 - 1}) + []
    figs[5] = (2 ** 31 - 1, 2, 100001, 100001, 2 ** 30 - 1)  # (the widest products the writer can meet)
    args = ["%d:%d:%d:%d:%d:%d:%d:%d:%d:%d" % (q, k % 4, d, le, le, t, rank, qn, qd, qr)
            for k, ((q, le, d), (t, rank, qn, qd, qr)) in enumerate(zip(pairs, figs))]
    out = subprocess.run([lines_check] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(pairs)
    plain, with_q = out[:len(pairs)], out[len(pairs):]
    for k, (a, b) in enumerate(zip(plain, with_q)):
        assert b == a + "," + fdr_ref.columns(figs[k]), (a, b)
        assert a.split(",")[0] == str(k) and a.rsplit(",", 5)[1] == str(pairs[k][2])
    assert with_q[0].endswith(",10,2,0.454545") and with_q[2].endswith(",10,4,1")  # (here query 0 has four pairs)
    assert with_q[5].endswith(",2147483647,2,%.6g" % (float((2 ** 31 - 1) * 100001) / float(100001 * (2 ** 30 - 1))))
