"""`ris -t -z N -H H [-D R]` without a GPU: tests/seqnull_ref.py's fold on hand-made summaries, the new refusals - made
before any GPU work - and the usage text."""
import os
import subprocess

import numpy as np
import pytest

import null_ref
import seqnull_ref

HERE = os.path.dirname(os.path.abspath(__file__))
QUERIES = os.path.join(HERE, "golden", "mix_q.fa")

Z = "-z (an empirical p-value per pair from N shuffled decoys)"
H = "-H (sequential p-values: a pair takes no more decoys once H of them reach its minimum energy)"
D = "-D (the decoys per round of the sequential p-values)"
REFUSALS = {
    "-t -H 2": f"Error: {H} needs {Z}",
    "-H 2": f"Error: {H} needs {Z}",
    "-t -G groups.tsv -P 3 -H 2": f"Error: {H} needs {Z}",
    "-t -A annot.tsv -F 3 -H 2": f"Error: {H} needs {Z}",
    "-k 2 -E 3 -H 2": f"Error: {H} needs {Z}",
    "-t -z 4 -D 2": f"Error: {D} needs {H}",
    "-t -D 2": f"Error: {D} needs {H}",
    "-t -z 4 -H 0": "Error: -H needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 4 -H 5": "Error: -H needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 4 -H x": "Error: -H needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 4 -H 2 -D 0": "Error: -D needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 4 -H 2 -D 5": "Error: -D needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 4 -H 2 -D many": "Error: -D needs an integer between 1 and the decoys per query (-z 4)",
    "-t -z 0 -H 1": "Error: -z needs an integer between 1 and 100000 (this build's limit)",
    "-t -z 4 -H 2 -n 2": f"Error: {Z} can't be combined with -n (the N best pairs per query)",
}


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, extra, **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", str(tmp_path / "nodb")] + extra,
                          capture_output=True, text=True, env=clean_env(**env))


@pytest.mark.parametrize("extra", list(REFUSALS))
def test_refused_before_any_gpu_work(tmp_path, extra):
    r = ris(tmp_path, extra.split())
    assert (r.stderr.splitlines() or [""])[0] == REFUSALS[extra]
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_refused_with_one_process_per_gpu(tmp_path):
    r = ris(tmp_path, ["-t", "-z", "4", "-H", "2"], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0] == f"Error: {Z} is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
    assert r.returncode == 1


def test_usage_names_the_switches():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-H INT" in text and "-D INT" in text and "Besag" in text


# ------------------------------------------------------------------------- the fold
def pairs(rows):
    """rows = [(query, db_id, e_min)] -> PAIR_DTYPE records"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e) in enumerate(rows):
        out[i] = (q, d, 1 + i % 3, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


REAL = {0: pairs([(0, 0, -10.0), (0, 1, -10.0), (0, 2, -10.0), (1, 0, -10.0), (1, 3, -10.0)])}
# per (owner, decoy): [(db_id, e_min)] - at or below -10 reaches the pair's minimum
HITS = {(0, 0): [(0, -11.0), (1, -10.0)], (0, 1): [(0, -12.0), (2, -9.0)], (0, 2): [(0, -13.0), (1, -10.5)], (0, 3): [(0, -9.0)],
        (0, 4): [(0, -14.0), (2, -10.0)], (1, 0): [(0, -10.0)], (1, 1): [], (1, 2): [(0, -9.5)], (1, 3): [], (1, 4): [(0, -15.0)]}
DECOYS = [(q, d, {0: pairs([(0, t, e) for t, e in rows])}) for (q, d), rows in HITS.items()]


def by_pair(recs):
    return {(int(r["query"]), int(r["db_id"])): (int(r["decoys"]), int(r["null_hits"]), int(r["null_le"]), float(r["null_min"])) for r in recs}


def test_fold_takes_each_pair_at_its_seen():
    """N = 5, H = 2, R = 2: the boundaries are 2, 4 and - a short last round - 5"""
    assert seqnull_ref.boundaries(5, 2) == [2, 4, 5] and seqnull_ref.boundaries(6, 2) == [2, 4, 6] and seqnull_ref.boundaries(3, 3) == [3]
    got = by_pair(seqnull_ref.fold(REAL, DECOYS, 5, 2, 2))
    assert got[(0, 0)] == (2, 2, 2, -12.0)       # NullLE(2) == H: retires at the first boundary; decoys 2 and 4 are not counted
    assert got[(0, 1)] == (4, 2, 2, -10.5)       # NullLE(2) == H - 1 does not retire; NullLE(4) == 2 does, at a later boundary
    assert got[(0, 2)] == (5, 2, 1, -10.0)       # one decoy in five reaches it: never retired
    assert got[(1, 0)] == (5, 3, 2, -15.0)       # reaches H in the short last round only: all N decoys, as without -H
    assert got[(1, 3)] == (5, 0, 0, np.inf)
    full = by_pair(null_ref.fold(REAL, DECOYS, 5))
    assert full[(0, 0)] == (5, 5, 4, -14.0) and full[(0, 1)] == (5, 2, 2, -10.5)
    assert {k: v for k, v in got.items() if v[0] == 5} == {k: v for k, v in full.items() if k in ((0, 2), (1, 0), (1, 3))}
    assert seqnull_ref.shows_every_case(REAL, DECOYS, 5, 2, 2) == {"first": True, "later": True, "never": True, "differs": True}


def test_fold_without_retiring_is_the_plain_fold():
    assert seqnull_ref.fold(REAL, DECOYS, 5, 5, 5).tobytes() == null_ref.fold(REAL, DECOYS, 5).tobytes()
    # every record is the record of `-z Seen`
    seq = seqnull_ref.fold(REAL, DECOYS, 5, 1, 1)
    for r in seq:
        b = int(r["decoys"])
        at = null_ref.fold(REAL, [x for x in DECOYS if x[1] < b], b)
        assert r.tobytes() in [x.tobytes() for x in at]
    assert by_pair(seq)[(0, 0)] == (1, 1, 1, -11.0) and by_pair(seq)[(0, 2)] == (5, 2, 1, -10.0)


def test_p_value_of_a_retired_pair_is_never_below_h_over_seen():
    """(NullLE + 1) / (Seen + 1) >= H / Seen whenever NullLE >= H and Seen >= H: the estimate errs to the large side"""
    for h, r in ((1, 1), (2, 2), (2, 1), (3, 2)):
        for rec in seqnull_ref.fold(REAL, DECOYS, 5, h, r):
            if rec["null_le"] >= h:
                assert null_ref.p_value(rec) >= h / float(rec["decoys"])
