"""The refusals of `ris` over its output switches -b -t -n -q -k, pinned exactly: every subset of the five, in two
argument orders, in one process and with one process per GPU (WORLD_SIZE=2 RANK=0).  They come before any GPU work.

The expected lines were recorded by running the binary of the commit BEFORE the command line was restructured around
one switch table (the parent of the commit that added this file) over these same combinations; they were not taken
from the restructured code.  Both argument orders gave the same line there."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

SWITCH = {"b": ["-b"], "t": ["-t"], "n": ["-n", "3"], "q": ["-q"], "k": ["-k", "3"]}

# the thirteen refusal texts
K_T = "Error: -k (the N best interaction sites per query) can't be combined with -t (per-pair summary lines)"
K_N = "Error: -k (the N best interaction sites per query) can't be combined with -n (the N best pairs per query)"
K_Q = "Error: -k (the N best interaction sites per query) can't be combined with -q (per-position profile lines)"
K_RANGE = "Error: -k needs an integer between 1 and 1024 (this build's limit)"
Q_T = "Error: -q (per-position profile lines) can't be combined with -t (per-pair summary lines)"
Q_N = "Error: -q (per-position profile lines) can't be combined with -n (the N best pairs per query)"
Q_B = "Error: -q (per-position profile lines) can't be combined with -b (binary hit records)"
T_B = "Error: -t (per-pair summary lines) can't be combined with -b (binary hit records)"
N_NEEDS_T = "Error: -n (the N best pairs per query) needs -t (per-pair summary lines)"
N_RANGE = "Error: -n needs an integer between 1 and 1024 (this build's limit)"
_RANKS = " is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
K_RANKS = "Error: -k (the N best interaction sites per query)" + _RANKS
Q_RANKS = "Error: -q (per-position profile lines)" + _RANKS
T_RANKS = "Error: -t (per-pair summary lines)" + _RANKS

# what marks a refusal of this family, for the combinations that are accepted
MARKS = ("can't be combined with", " needs -", "needs an integer", "is not supported with one process per GPU")

# switches given -> (first line of stderr in one process, with one process per GPU); None: accepted
EXPECTED = {
    "": (None, None),
    "b": (None, None),
    "t": (None, T_RANKS),
    "bt": (T_B, T_B),
    "n": (N_NEEDS_T, N_NEEDS_T),
    "bn": (N_NEEDS_T, N_NEEDS_T),
    "tn": (None, T_RANKS),
    "btn": (T_B, T_B),
    "q": (None, Q_RANKS),
    "bq": (Q_B, Q_B),
    "tq": (Q_T, Q_T),
    "btq": (Q_T, Q_T),
    "nq": (Q_N, Q_N),
    "bnq": (Q_N, Q_N),
    "tnq": (Q_T, Q_T),
    "btnq": (Q_T, Q_T),
    "k": (None, K_RANKS),
    "bk": (None, K_RANKS),
    "tk": (K_T, K_T),
    "btk": (K_T, K_T),
    "nk": (K_N, K_N),
    "bnk": (K_N, K_N),
    "tnk": (K_T, K_T),
    "btnk": (K_T, K_T),
    "qk": (K_Q, K_Q),
    "bqk": (K_Q, K_Q),
    "tqk": (K_T, K_T),
    "btqk": (K_T, K_T),
    "nqk": (K_N, K_N),
    "bnqk": (K_N, K_N),
    "tnqk": (K_T, K_T),
    "btnqk": (K_T, K_T),
}

# values of -n / -k that are out of range, beside one other switch: the range message comes after the combination
# messages for -k, and after "needs -t" (and -t's own combinations) for -n
OUT_OF_RANGE = {
    "-k 0": K_RANGE,
    "-k 0 -b": K_RANGE,
    "-k 1025 -b": K_RANGE,
    "-k 0 -t": K_T,
    "-k 0 -n 3": K_N,
    "-k abc -q": K_Q,
    "-n 0": N_NEEDS_T,
    "-n 0 -b": N_NEEDS_T,
    "-t -n 0": N_RANGE,
    "-t -n 1025": N_RANGE,
    "-t -n 0 -b": T_B,
    "-n 0 -q": Q_N,
    "-n 0 -k 3": K_N,
    "-n 0 -k 0": K_N,
}


def ris(tmp_path, extra, ranks):
    from priblast_amd import capi
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    if ranks:
        env.update(WORLD_SIZE="2", RANK="0")
    return subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"),
                           "-d", str(tmp_path / "nodb")] + extra, capture_output=True, text=True, env=env)


def check(tmp_path, r, want):
    first = (r.stderr.splitlines() or [""])[0]
    if want is None:  # accepted: what follows depends on whether a device is present
        assert not any(m in r.stderr for m in MARKS), r.stderr
        return
    assert first == want
    assert r.returncode != 0
    assert not (tmp_path / "out").exists()


def test_the_table_covers_every_subset():
    assert len(EXPECTED) == 32
    assert set(EXPECTED) == {"".join(c for i, c in enumerate("btnqk") if mask >> i & 1) for mask in range(32)}


@pytest.mark.parametrize("ranks", [False, True], ids=["one_process", "world_size_2"])
@pytest.mark.parametrize("reverse", [False, True], ids=["as_given", "reversed"])
@pytest.mark.parametrize("given", list(EXPECTED), ids=[k or "none" for k in EXPECTED])
def test_refusal_of_every_switch_combination(tmp_path, given, reverse, ranks):
    groups = [SWITCH[c] for c in given]
    extra = sum(groups[::-1] if reverse else groups, [])
    check(tmp_path, ris(tmp_path, extra, ranks), EXPECTED[given][ranks])


@pytest.mark.parametrize("extra", list(OUT_OF_RANGE))
def test_range_message_keeps_its_place(tmp_path, extra):
    check(tmp_path, ris(tmp_path, extra.split(), False), OUT_OF_RANGE[extra])
