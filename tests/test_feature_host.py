"""`ris -t -A FILE` without a GPU: the reference fold (tests/feature_ref.py) on tiny hand-made cases, the annotation that
the search tests use checked against the committed golden hits, and the refusals of the command line - a faulty annotation
file, -A without -t, -A with a switch it does not go with - each of which ends the run before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import feature_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


# ------------------------------------------------------------------------- the reference
def hits_of(rows, start_pos, length):
    """rows = [(query, db_id, lo, hi, e_tot)] on targets of one length laid out one after the other -> (HIT_DTYPE, pairs)"""
    from priblast_amd import capi
    hits = np.zeros(len(rows), capi.HIT_DTYPE)
    bp = np.zeros((2 * len(rows), 2), np.int32)
    for i, (q, d, lo, hi, e) in enumerate(rows):
        bp[2 * i] = (i, start_pos[d] + length - 1 - lo)
        bp[2 * i + 1] = (i + 1, start_pos[d] + length - 1 - hi)
        hits[i]["query"], hits[i]["db_id"], hits[i]["e_tot"], hits[i]["e_acc"], hits[i]["e_hyb"] = q, d, e, 1.0 + i, e - 1.0 - i
        hits[i]["bp_count"], hits[i]["bp_offset"] = 2, 2 * i
    return hits, bp


def test_the_reference_folds_hits_into_their_features():
    start_pos, length = [0, 11, 22], 10
    seqs = [[(s, length) for s in start_pos]]
    annot = [(0, 0, 4, 6), (0, 0, 0, 9), (0, 2, 0, 0), (0, 0, 4, 6)]
    rows = [(0, 0, 0, 3, -5.0), (0, 0, 3, 4, -7.0), (0, 0, 5, 5, -7.0), (0, 1, 2, 3, -9.0), (1, 2, 1, 4, -2.0), (1, 2, 0, 2, -0.5)]
    got, un = feature_ref.fold({0: hits_of(rows, start_pos, length)}, annot, seqs)
    # the features of target 0 by (start, end, index): 1, then 0 and its duplicate 3
    assert [(int(r["query"]), int(r["db_id"]), int(r["feature"]), int(r["hits"]), int(r["inside"])) for r in got] == \
        [(0, 0, 1, 3, 3), (0, 0, 0, 2, 1), (0, 0, 3, 2, 1), (1, 2, 2, 1, 0)]
    assert un == 2  # the hit on target 1, which has no feature, and the one that starts behind position 0 of target 2
    assert float(got[0]["e_min"]) == -7.0 and got[0]["bp_first"].tolist() == [1, start_pos[0] + length - 1 - 3]  # the first of the two
    assert float(got[0]["e_sum"]) == -19.0 and float(got[1]["e_sum"]) == -14.0
    assert float(got[3]["e_acc"]) == 6.0 and (got["page"] == 0).all()


def test_the_reference_adds_left_to_right_and_keeps_the_first_zero():
    start_pos, length = [0], 10
    rows = [(0, 0, 1, 2, 1e16), (0, 0, 1, 2, 1.0), (0, 0, 1, 2, -1e16), (0, 0, 1, 2, 1.0), (1, 0, 1, 2, 0.0), (1, 0, 1, 2, -0.0)]
    got, un = feature_ref.fold({0: hits_of(rows, start_pos, length)}, [(0, 0, 0, 9)], [[(0, length)]])
    assert un == 0 and float(got[0]["e_sum"]) == 1.0 and not np.signbit(got[1]["e_min"])


def test_the_reference_folds_text_lines():
    lines = ["0,qa,30,t1,40,1.5,-9.5,-8,(3:20) (4:19) (5:18) ", "1,qa,30,t1,40,2.5,-12.5,-10,(7:9) (8:8) ",
             "2,qa,30,t2,50,0.5,-8.75,-8.25,(1:30) (2:31) "]
    want, un = feature_ref.fold_lines(lines, {"t1": [(15, 39, "cds"), (0, 8, "utr5"), (9, 18, "start")]})
    assert un == 1
    assert want == [["qa", "30", "t1", "40", "1", "-10", -10.0, "2.5", "-12.5", "(7-8:9-8) ", "utr5", "0-8", "0"],
                    ["qa", "30", "t1", "40", "2", "-10", -18.0, "2.5", "-12.5", "(7-8:9-8) ", "start", "9-18", "0"],
                    ["qa", "30", "t1", "40", "1", "-8", -8.0, "1.5", "-9.5", "(3-5:20-18) ", "cds", "15-39", "1"]]
    assert feature_ref.same_lines(["0,qa,30,t1,40,1,-10,-10,2.5,-12.5,(7-8:9-8) ,utr5,0-8,0", "1,qa,30,t1,40,2,-10,-18,2.5,-12.5,(7-8:9-8) ,start,9-18,0",
                                   "2,qa,30,t1,40,1,-8,-8,1.5,-9.5,(3-5:20-18) ,cds,15-39,1"], want)
    assert not feature_ref.same_lines(["0,qa,30,t1,40,1,-10,-10.1,2.5,-12.5,(7-8:9-8) ,utr5,0-8,1"], want[:1])


@pytest.mark.parametrize("tag", ["mix", "edge"])
def test_the_golden_annotation_meets_the_search_tests_preconditions(tag):
    """Against the reference's own hits the annotation of test_gpu_feature.py and test_feature_cli.py yields at least one hit
    that straddles two features, one inside a nested feature, one that touches a feature by exactly one position, one
    unassigned hit, and one target with hits and no feature."""
    with open(os.path.join(GOLDEN, f"{tag}_ris_s1.out")) as f:
        lines = f.read().splitlines()[2:]
    annot = feature_ref.golden_annotation(lines)
    count = feature_ref.preconditions(lines, annot)
    assert all(v >= 1 for v in count.values()), count
    lengths = {l.split(",")[2]: int(l.split(",")[3]) for l in lines}
    assert all(0 <= s <= e < lengths[t] for t, s, e, _ in annot)


# ------------------------------------------------------------------------- the command line
def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", db] + extra, capture_output=True, text=True,
                          env=clean_env(**env))


SHAPE = "expected target name, start, end and feature name, separated by tabs (0-based, inclusive coordinates)"
# (mdb1 has 141 bases)
FILES = {
    "three_fields": ("mdb1\t3\t9\n", 1, SHAPE),
    "five_fields": ("# a comment\n\nmdb1\t3\t9\tcds\nmdb1\t3\t9\tcds\textra\n", 4, SHAPE),
    "not_a_number": ("mdb1\t3\t9\tcds\r\nmdb1\tx\t9\tcds\r\n", 2, SHAPE),
    "negative": ("mdb1\t-3\t9\tcds\n", 1, SHAPE),
    "empty_name": ("mdb1\t3\t9\t\n", 1, SHAPE),
    "unknown_target": ("mdb1\t3\t9\tcds\nmdb99\t3\t9\tcds\n", 2, 'no database sequence is named "mdb99"'),
    "start_behind_end": ("mdb1\t10\t9\tcds\n", 1, "start 10 is behind end 9"),
    "end_outside": ("mdb1\t0\t140\tcds\nmdb1\t0\t141\tcds\n", 2, 'end 141 is outside "mdb1" (length 141)'),
}


def check_file_refusal(tmp_path, golden_dir, case):
    text, lineno, why = FILES[case]
    path = tmp_path / "features.tsv"
    path.write_bytes(text.encode())
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-A", str(path)])
    assert (r.stderr.splitlines() or [""])[0] == f"Error: annotation file {path} line {lineno}: {why}"
    assert r.returncode == 1 and not (tmp_path / "out").exists()


@pytest.mark.parametrize("case", list(FILES))
def test_a_faulty_annotation_file_is_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    check_file_refusal(tmp_path, golden_dir, case)


def test_an_unreadable_annotation_file_is_refused(tmp_path, golden_dir):
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-A", str(tmp_path / "missing.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == "Error: can't open the annotation file (-A): " + str(tmp_path / "missing.tsv")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


A = "-A (one line per query-feature pair)"
SWITCHES = {
    "without_t": ([], "Error: " + A + " needs -t (per-pair summary lines)"),
    "n": (["-t", "-n", "3"], "Error: " + A + " can't be combined with -n (the N best pairs per query)"),
    "z": (["-t", "-z", "4"], "Error: " + A + " can't be combined with -z (an empirical p-value per pair from N shuffled decoys)"),
    "k": (["-k", "3"], "Error: " + A + " can't be combined with -k (the N best interaction sites per query)"),
    "q": (["-q"], "Error: " + A + " can't be combined with -q (per-position profile lines)"),
    "r": (["-r", "3"], "Error: " + A + " can't be combined with -r (the N best queries per target)"),
    "c": (["-c", "2"], "Error: " + A + " can't be combined with -c (the regions of each target bound by at least D queries)"),
    "b": (["-b"], "Error: " + A + " can't be combined with -b (binary hit records)"),
    "G": (["-t", "-G", "GROUPS"], "Error: " + A + " can't be combined with -G (one line per query-group pair)"),
    "P": (["-t", "-P", "4"], "Error: " + A + " can't be combined with -P (an empirical p-value per query-group pair from N shuffled decoys)"),
    "E": (["-k", "3", "-E", "4"], "Error: " + A + " can't be combined with -k (the N best interaction sites per query)"),
    "E_alone": (["-t", "-E", "4"], "Error: " + A + " can't be combined with -E (an E-value and a q-value per interaction site from N pooled decoys "
                                   "per query)"),
    "R": (["-t", "-R", "4"], "Error: " + A + " can't be combined with -R (the N best queries per group)"),
}


def check_switch_refusal(tmp_path, golden_dir, case):
    extra, want = SWITCHES[case]
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    extra = [str(tmp_path / "groups.tsv") if x == "GROUPS" else x for x in extra]
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra + ["-A", str(tmp_path / "features.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


@pytest.mark.parametrize("case", list(SWITCHES))
def test_switch_combinations_are_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    check_switch_refusal(tmp_path, golden_dir, case)


def test_one_process_per_gpu_is_refused(tmp_path, golden_dir):
    (tmp_path / "features.tsv").write_text("mdb1\t3\t9\tcds\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-A", str(tmp_path / "features.tsv")], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0].startswith("Error: " + A + " is not supported with one process per GPU (WORLD_SIZE > 1)")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-A STR" in text and "target name, a tab, start, a tab, end, a tab, feature name" in text
