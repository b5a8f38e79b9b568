"""`ris -t -A FILE -F N` without a GPU: the reference fold (tests/fnull_ref.py) on hand-made cases, and the refusals of the
command line - -F without -A, with a switch that -A does not go with, with a count outside its range, a bad seed, one
process per GPU - each of which ends the run before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import fnull_ref
from test_feature_host import hits_of

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


# ------------------------------------------------------------------------- the reference
START, LENGTH = [0, 11, 22], 10
SEQS = [[(s, LENGTH) for s in START]]
ANNOT = [(0, 0, 0, 4), (0, 0, 3, 9), (0, 2, 0, 9)]  # two overlapping features on target 0, none on target 1, one on target 2


def columns(recs):
    return [(int(r["query"]), int(r["feature"]), int(r["null_hits"]), int(r["null_le"]), float(r["null_min"])) for r in recs]


def batch(rows, owner, decoy):
    return {0: hits_of(rows, START, LENGTH)}, np.array(owner, np.int32), np.array(decoy, np.int32)


def test_a_decoy_counts_in_every_kept_feature_its_hit_meets_and_nowhere_else():
    real = {0: hits_of([(0, 0, 0, 2, -10.0), (0, 0, 5, 6, -9.0), (1, 2, 1, 2, -5.0)], START, LENGTH)}
    decoys = [batch([(0, 0, 3, 4, -9.5),    # decoy 0 of query 0 meets both features of target 0: above -10, below -9
                     (1, 0, 5, 9, -9.0),    # decoy 1 of query 0: only feature 1, equal to e_obs
                     (1, 1, 0, 9, -99.0),   # ... and a target without features
                     (2, 2, 0, 0, -99.0),   # decoy 2 of query 0 on feature 2, which is kept for query 1 only
                     (3, 0, 0, 9, -99.0)],  # decoy 0 of query 1 on features that are kept for query 0 only
                    [0, 0, 0, 1], [0, 1, 2, 0]),
              batch([(0, 2, 9, 9, -4.0), (0, 2, 0, 0, -4.5)], [1, 1], [1, 2])]  # decoy 1 of query 1: two hits, the minimum counts
    got = fnull_ref.fold_hits(real, decoys, ANNOT, SEQS, 3)
    assert columns(got) == [(0, 0, 1, 0, -9.5), (0, 1, 2, 2, -9.5), (1, 2, 1, 0, -4.5)]
    assert [int(r["decoys"]) for r in got] == [3, 3, 3] and [float(r["e_min"]) for r in got] == [-10.0, -9.0, -5.0]
    # the observed side is the feature table's record, field for field
    import feature_ref
    kept, _ = feature_ref.fold(real, ANNOT, SEQS)
    assert all(got[n].tolist() == kept[n].tolist() for n in kept.dtype.names)


def test_the_zeros_are_equal_and_a_feature_without_a_decoy_hit_reports_infinity():
    real = {0: hits_of([(0, 0, 0, 0, 0.0), (0, 2, 0, 0, -2.0)], START, LENGTH)}
    got = fnull_ref.fold_hits(real, [batch([(0, 0, 4, 4, -0.0)], [0], [0])], ANNOT[:1] + ANNOT[2:], SEQS, 1)
    assert columns(got) == [(0, 0, 1, 1, 0.0), (0, 1, 0, 0, np.inf)] and not np.signbit(got[0]["null_min"])


def test_spans_that_touch_by_one_position_and_miss_by_one():
    real = {0: hits_of([(0, 0, 3, 9, -5.0)], START, LENGTH)}
    annot = [(0, 0, 3, 6)]
    rows = [(0, 0, 0, 3, -6.0), (1, 0, 6, 9, -7.0), (2, 0, 0, 2, -8.0), (3, 0, 7, 9, -9.0)]
    got = fnull_ref.fold_hits(real, [batch(rows, [0] * 4, [0, 1, 2, 3])], annot, SEQS, 4)
    assert columns(got) == [(0, 0, 2, 2, -7.0)]


def test_the_reference_folds_text_lines():
    real = ["0,qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ,cds,0-20,1", "1,qa,30,t0,40,1,-12,-12,1,-13,(1-5:9-3) ,utr,21-39,1",
            "2,qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) ,cds,0-20,0"]
    decoy = ["0,qa_d0,30,t0,40,1,-12,-12,1,-13,(1-5:9-3) ,cds,0-20,1", "1,qa_d0,30,t0,40,1,-12.5,-12,1,-13,(1-5:9-3) ,utr,21-39,1",
             "2,qa_d1,30,t2,40,1,-50,-50,1,-13,(1-5:9-3) ,cds,0-20,1", "3,qb_d1,20,t2,40,1,-2,-2,1,-4,(1-5:9-3) ,cds,0-20,1",
             "4,qa_d1,30,t0,40,1,-9,-9,1,-13,(1-5:9-3) ,cds,0-20,1"]
    decoy_of = {"qa_d0": ("qa", 0), "qa_d1": ("qa", 1), "qb_d0": ("qb", 0), "qb_d1": ("qb", 1)}
    got = fnull_ref.fold_lines(real, decoy, decoy_of, 2)
    assert got == ["qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ,cds,0-20,1,2,2,1,-12,0.666667",
                   "qa,30,t0,40,1,-12,-12,1,-13,(1-5:9-3) ,utr,21-39,1,2,1,1,-12.5,0.666667",
                   "qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) ,cds,0-20,0,2,1,0,-2,0.333333"]
    assert fnull_ref.fold_lines(real[:1], [], decoy_of, 2) == [real[0].split(",", 1)[1] + ",2,0,0,NA,0.333333"]


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


F = "-F (an empirical p-value per query-feature pair from N shuffled decoys)"
LIMIT = "Error: -F needs an integer between 1 and 100000 (this build's limit)"
# name: (switches, with -A FILE, the first line of stderr)
SWITCHES = {
    "without_A": (["-t", "-F", "4"], False, "Error: " + F + " needs -A (one line per query-feature pair)"),
    "without_A_or_t": (["-F", "4"], False, "Error: " + F + " needs -A (one line per query-feature pair)"),
    "without_t": (["-F", "4"], True, "Error: -A (one line per query-feature pair) needs -t (per-pair summary lines)"),
    "n": (["-t", "-F", "4", "-n", "3"], True, "Error: " + F + " can't be combined with -n (the N best pairs per query)"),
    "z": (["-t", "-F", "4", "-z", "4"], True, "Error: " + F + " can't be combined with -z (an empirical p-value per pair from N shuffled decoys)"),
    "k": (["-F", "4", "-k", "3"], True, "Error: " + F + " can't be combined with -k (the N best interaction sites per query)"),
    "q": (["-F", "4", "-q"], True, "Error: " + F + " can't be combined with -q (per-position profile lines)"),
    "r": (["-F", "4", "-r", "3"], True, "Error: " + F + " can't be combined with -r (the N best queries per target)"),
    "c": (["-F", "4", "-c", "2"], True, "Error: " + F + " can't be combined with -c (the regions of each target bound by at least D queries)"),
    "b": (["-t", "-F", "4", "-b"], True, "Error: " + F + " can't be combined with -b (binary hit records)"),
    "G": (["-t", "-F", "4", "-G", "GROUPS"], True, "Error: " + F + " can't be combined with -G (one line per query-group pair)"),
    "P": (["-t", "-F", "4", "-P", "4"], True,
          "Error: " + F + " can't be combined with -P (an empirical p-value per query-group pair from N shuffled decoys)"),
    "E": (["-t", "-F", "4", "-E", "4"], True,
          "Error: " + F + " can't be combined with -E (an E-value and a q-value per interaction site from N pooled decoys per query)"),
    "R": (["-t", "-F", "4", "-R", "4"], True, "Error: " + F + " can't be combined with -R (the N best queries per group)"),
    "zero": (["-t", "-F", "0"], True, LIMIT),
    "too_many": (["-t", "-F", "100001"], True, LIMIT),
    "no_count": (["-t", "-F", "many"], True, LIMIT),
    "bad_seed": (["-t", "-F", "4", "-Z", "-1"], True, "Error: -Z needs a non-negative integer"),
}


def check_switch_refusal(tmp_path, golden_dir, case, **env):
    extra, with_annot, want = SWITCHES[case]
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    extra = [str(tmp_path / "groups.tsv") if x == "GROUPS" else x for x in extra]
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra + (["-A", str(tmp_path / "features.tsv")] if with_annot else []), **env)
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


@pytest.mark.parametrize("case", list(SWITCHES))
def test_switch_combinations_are_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    check_switch_refusal(tmp_path, golden_dir, case)


def test_the_seed_switch_goes_with_F_and_still_needs_a_switch_that_makes_decoys(tmp_path, golden_dir):
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-Z", "5", "-A", str(tmp_path / "features.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == ("Error: -Z (the seed of the decoys' shuffles) needs -z (an empirical p-value per pair from N "
                                                  "shuffled decoys)")
    assert r.returncode == 1 and not (tmp_path / "out").exists()
    # with -F the seed passes the switch table: the run is refused by the next check, here the one for one process per GPU
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-Z", "5", "-F", "4", "-A", str(tmp_path / "features.tsv")], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0].startswith("Error: " + F + " is not supported with one process per GPU")


def test_one_process_per_gpu_is_refused(tmp_path, golden_dir):
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-F", "4", "-A", str(tmp_path / "features.tsv")], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0] == "Error: " + F + (" is not supported with one process per GPU (WORLD_SIZE > 1); use "
                                                                  "PRB_DEVICES=0,1,.. in one process")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-F INT" in text and "with -z or -P, with -F, or with -E" in text and "empirical p-value per query-feature pair" in text
