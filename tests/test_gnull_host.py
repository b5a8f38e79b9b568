"""`ris -t -G FILE -P N` without a GPU: the reference fold (tests/gnull_ref.py) on hand-made lists, and the refusals of the
command line, each of which ends the run before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import gnull_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


def pairs(rows):
    """rows = [(query, db_id, e_min, hits)] -> PAIR_DTYPE records with every other field filled in recognisably"""
    from priblast_amd import capi
    out = np.zeros(len(rows), capi.PAIR_DTYPE)
    for i, (q, d, e, h) in enumerate(rows):
        out[i] = (q, d, h, e, e - 1.5, 0.25 * i, e - 0.25 * i, (i, i + 1), (i + 2, i + 3))
    return out


# ------------------------------------------------------------------------- the reference
MAPS = [[0, 1, 1, 2, 3], [0, 4, 0]]  # group 0 = {page 0: t0; page 1: t0, t2}, group 1 = {page 0: t1, t2}, singletons 2, 3, 4


def columns(recs):
    return [(int(r["query"]), int(r["group"]), int(r["null_hits"]), int(r["null_le"]), float(r["null_min"])) for r in recs]


def test_a_decoy_counts_once_per_group_and_on_members_the_query_did_not_hit():
    real = {0: pairs([(0, 0, -10.0, 2), (0, 1, -9.0, 1)]), 1: pairs([(1, 1, -5.0, 1)])}
    decoys = [(0, 0, {0: pairs([(0, 0, -11.0, 1)]), 1: pairs([(0, 0, -12.0, 1), (0, 2, -10.5, 1)])}),  # below e_obs on three members of group 0
              (0, 1, {1: pairs([(0, 2, -10.0, 1)])}),  # only on a member the real query did not hit, and equal to e_obs
              (0, 2, {0: pairs([(0, 2, -8.0, 1), (0, 4, -30.0, 1)])}),  # group 1 above e_obs; group 3 is not observed for query 0
              (1, 0, {1: pairs([(0, 1, -4.0, 1)])}), (1, 1, {}), (1, 2, {})]
    got = gnull_ref.fold(real, MAPS, 5, decoys, 3)
    assert columns(got) == [(0, 0, 2, 2, -12.0), (0, 1, 1, 0, -8.0), (1, 4, 1, 0, -4.0)]
    assert [int(r["decoys"]) for r in got] == [3, 3, 3] and got[0]["e_min"] == -10.0 and int(got[0]["members"]) == 1
    # the observed side is the group table's record
    import group_ref
    assert got[["query", "db_id", "e_min", "page", "group", "members", "rank", "group_hits"]].tolist() == \
        group_ref.fold(real, MAPS, 5)[["query", "db_id", "e_min", "page", "group", "members", "rank", "group_hits"]].tolist()


def test_the_zeros_are_equal_and_a_group_without_a_decoy_hit_reports_infinity():
    real = {0: pairs([(0, 0, 0.0, 1), (0, 3, -2.0, 1)])}
    decoys = [(0, 0, {0: pairs([(0, 0, -0.0, 1)])})]
    got = gnull_ref.fold(real, MAPS, 5, decoys, 1)
    assert columns(got) == [(0, 0, 1, 1, 0.0), (0, 2, 0, 0, np.inf)] and not np.signbit(got[0]["null_min"])


def test_with_n_only_the_kept_groups_count():
    real = {0: pairs([(0, 0, -10.0, 1), (0, 1, -12.0, 1), (0, 3, -11.0, 1)])}
    decoys = [(0, 0, {0: pairs([(0, 0, -20.0, 1), (0, 1, -20.0, 1), (0, 3, -20.0, 1)])})]
    got = gnull_ref.fold(real, MAPS, 5, decoys, 1, n=2)
    assert columns(got) == [(0, 1, 1, 1, -20.0), (0, 2, 1, 1, -20.0)] and [int(r["rank"]) for r in got] == [0, 1]


def test_the_reference_folds_text_lines():
    real = ["0,qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ", "1,qa,30,t1,40,1,-12,-12,1,-13,(1-5:9-3) ", "2,qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) "]
    decoy = ["0,qa_d0,30,t2,40,1,-12,-12,1,-13,(1-5:9-3) ", "1,qa_d0,30,t1,40,1,-12.5,-12,1,-13,(1-5:9-3) ", "2,qa_d1,30,t3,40,1,-50,-50,1,-13,(1-5:9-3) ",
             "3,qb_d1,20,t1,40,1,-2,-2,1,-4,(1-5:9-3) "]
    decoy_of = {"qa_d0": ("qa", 0), "qa_d1": ("qa", 1), "qb_d0": ("qb", 0), "qb_d1": ("qb", 1)}
    got = gnull_ref.fold_lines(real, decoy, decoy_of, ["t0", "t1", "t2", "t3"], {"t1": "g", "t2": "g"}, 2)
    assert got == ["qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ,t0,1,1,2,2,0,0,NA,0.333333",
                   "qa,30,t1,40,1,-12,-12,1,-13,(1-5:9-3) ,g,1,2,1,2,1,1,-12.5,0.666667",
                   "qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) ,g,1,2,1,2,1,0,-2,0.333333"]


# ------------------------------------------------------------------------- refusals (no GPU)
def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", db] + extra, capture_output=True, text=True,
                          env=clean_env(**env))


P = "-P (an empirical p-value per query-group pair from N shuffled decoys)"
LIMIT = "Error: -P needs an integer between 1 and 100000 (this build's limit)"
SWITCHES = {
    "without_G": (["-t", "-P", "4"], False, "Error: " + P + " needs -G (one line per query-group pair)"),
    "without_G_or_t": (["-P", "4"], False, "Error: " + P + " needs -G (one line per query-group pair)"),
    "z": (["-t", "-P", "4", "-z", "4"], True, "Error: " + P + " can't be combined with -z (an empirical p-value per pair from N shuffled decoys)"),
    "k": (["-P", "4", "-k", "3"], True, "Error: " + P + " can't be combined with -k (the N best interaction sites per query)"),
    "q": (["-P", "4", "-q"], True, "Error: " + P + " can't be combined with -q (per-position profile lines)"),
    "r": (["-P", "4", "-r", "3"], True, "Error: " + P + " can't be combined with -r (the N best queries per target)"),
    "c": (["-P", "4", "-c", "2"], True, "Error: " + P + " can't be combined with -c (the regions of each target bound by at least D queries)"),
    "b": (["-t", "-P", "4", "-b"], True, "Error: " + P + " can't be combined with -b (binary hit records)"),
    "zero": (["-t", "-P", "0"], True, LIMIT),
    "too_many": (["-t", "-P", "100001"], True, LIMIT),
    "no_count": (["-t", "-P", "many"], True, LIMIT),
    "bad_seed": (["-t", "-P", "4", "-Z", "-1"], True, "Error: -Z needs a non-negative integer"),
}


@pytest.mark.parametrize("case", list(SWITCHES))
def test_switch_combinations_are_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    extra, with_groups, want = SWITCHES[case]
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra + (["-G", str(tmp_path / "groups.tsv")] if with_groups else []))
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_the_seed_switch_still_needs_a_switch_that_makes_decoys(tmp_path, golden_dir):
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-Z", "5", "-G", str(tmp_path / "groups.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == ("Error: -Z (the seed of the decoys' shuffles) needs -z (an empirical p-value per pair from N "
                                                  "shuffled decoys)")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_one_process_per_gpu_is_refused(tmp_path, golden_dir):
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-P", "4", "-G", str(tmp_path / "groups.tsv")], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0] == "Error: " + P + (" is not supported with one process per GPU (WORLD_SIZE > 1); use "
                                                                  "PRB_DEVICES=0,1,.. in one process")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-P INT" in text and "with -z or -P" in text and "p-values per group" not in text and "not implemented" in text
