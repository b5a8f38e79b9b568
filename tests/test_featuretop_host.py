"""`ris -t -A FILE -N K` without a GPU: the yardstick of the ranked cut (tests/featuretop_ref.py) on a hand-made array, and
the refusals of the command line - -N without -A, -N with what -A does not go with, a value out of range - each of which
ends the run before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import featuretop_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


# ------------------------------------------------------------------------- the yardstick
def test_select_keeps_the_first_n_of_a_stable_sort_per_query():
    from priblast_amd import capi
    rows = [(0, 7, -3.0), (0, 1, -9.0), (0, 4, -9.0), (0, 2, -5.0), (2, 3, -1.0), (2, 9, -2.0), (3, 5, -4.0)]  # (query, feature, e_min)
    recs = np.zeros(len(rows), capi.FEATURE_DTYPE)
    for i, (q, f, e) in enumerate(rows):
        recs[i]["query"], recs[i]["feature"], recs[i]["e_min"], recs[i]["inside"] = q, f, e, i
    pick = lambda n: [(int(r["query"]), int(r["feature"])) for r in featuretop_ref.select(recs, n)]
    assert pick(1) == [(0, 1), (2, 9), (3, 5)]                      # of the tie at -9 the earlier record
    assert pick(2) == [(0, 1), (0, 4), (2, 9), (2, 3), (3, 5)]      # the cut inside ... and behind the tie
    assert pick(3) == [(0, 1), (0, 4), (0, 2), (2, 9), (2, 3), (3, 5)]
    assert pick(1024) == [(0, 1), (0, 4), (0, 2), (0, 7), (2, 9), (2, 3), (3, 5)]
    kept = featuretop_ref.select(recs, 2)
    assert kept[1].tobytes() == recs[2].tobytes() and kept.dtype == recs.dtype  # field for field
    assert len(featuretop_ref.select(recs[:0], 3)) == 0


def test_select_lines_accepts_a_ranked_cut_and_names_what_is_wrong_with_another():
    line = lambda i, q, t, e, f: f"{i},{q},30,{t},40,1,{e},{e},1.5,-9.5,(3-5:20-18) ,{f},0-8,0"
    full = [line(0, "qa", "t1", -8, "a"), line(1, "qa", "t1", -12, "b"), line(2, "qa", "t2", -12, "c"), line(3, "qb", "t1", -9, "a")]
    cut = lambda *rows: [f"{k}," + full[i].split(",", 1)[1] for k, i in enumerate(rows)]
    assert featuretop_ref.select_lines(cut(1, 2, 3), full, 2) is None
    assert featuretop_ref.select_lines(cut(2, 1, 3), full, 2) is None  # (equal printed energies: either order)
    assert featuretop_ref.select_lines(cut(1, 3), full, 1) is None
    assert "want min(2, 3)" in featuretop_ref.select_lines(cut(1, 3), full, 2)
    assert "decrease with rank" in featuretop_ref.select_lines(cut(0, 1, 3), full, 2)
    assert "lower energy" in featuretop_ref.select_lines(cut(0, 3), full, 1)
    assert "not a line" in featuretop_ref.select_lines(cut(1, 3)[:1] + ["1," + full[3].split(",", 1)[1].replace("qb", "qa")], full, 2)
    assert "Ids" in featuretop_ref.select_lines(full[1:3] + full[3:], full, 2)


# ------------------------------------------------------------------------- the command line
def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, **env):
    from priblast_amd import capi
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    extra = [str(tmp_path / "groups.tsv") if x == "GROUPS" else str(tmp_path / "features.tsv") if x == "FEATURES" else x for x in extra]
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", db] + extra, capture_output=True, text=True,
                          env=clean_env(**env))


A = "-A (one line per query-feature pair)"
N = "-N (the N best features per query)"
RANGE = "Error: -N needs an integer between 1 and 1024 (this build's limit)"
SWITCHES = {
    "without_A": (["-t", "-N", "3"], "Error: " + N + " needs " + A),
    "without_t": (["-A", "FEATURES", "-N", "3"], "Error: " + A + " needs -t (per-pair summary lines)"),
    "zero": (["-t", "-A", "FEATURES", "-N", "0"], RANGE),
    "too_many": (["-t", "-A", "FEATURES", "-N", "1025"], RANGE),
    "not_a_number": (["-t", "-A", "FEATURES", "-N", "x"], RANGE),
    "n": (["-t", "-n", "3", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -n (the N best pairs per query)"),
    "z": (["-t", "-z", "4", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -z (an empirical p-value per pair from N shuffled decoys)"),
    "k": (["-k", "3", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -k (the N best interaction sites per query)"),
    "q": (["-q", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -q (per-position profile lines)"),
    "r": (["-r", "3", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -r (the N best queries per target)"),
    "c": (["-c", "2", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -c (the regions of each target bound by at least D queries)"),
    "b": (["-b", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -b (binary hit records)"),
    "G": (["-t", "-G", "GROUPS", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -G (one line per query-group pair)"),
    "P": (["-t", "-P", "4", "-A", "FEATURES", "-N", "3"],
          "Error: " + A + " can't be combined with -P (an empirical p-value per query-group pair from N shuffled decoys)"),
    "E": (["-t", "-E", "4", "-A", "FEATURES", "-N", "3"],
          "Error: " + A + " can't be combined with -E (an E-value and a q-value per interaction site from N pooled decoys per query)"),
    "R": (["-t", "-R", "4", "-A", "FEATURES", "-N", "3"], "Error: " + A + " can't be combined with -R (the N best queries per group)"),
}


@pytest.mark.parametrize("case", list(SWITCHES))
def test_switch_combinations_and_values_are_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    extra, want = SWITCHES[case]
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra)
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


@pytest.mark.parametrize("extra", [[], ["-F", "4"]])
def test_one_process_per_gpu_is_refused(tmp_path, golden_dir, extra):
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-A", "FEATURES", "-N", "3"] + extra, WORLD_SIZE="2", RANK="0")
    first = (r.stderr.splitlines() or [""])[0]
    assert "is not supported with one process per GPU (WORLD_SIZE > 1)" in first and first.startswith("Error: -F (" if extra else "Error: " + A)
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-N INT" in text and "lowest minimum interaction energy per query" in text
