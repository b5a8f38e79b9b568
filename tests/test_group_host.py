"""`ris -t -G FILE` without a GPU: the reference fold (tests/group_ref.py) on hand-made lists, and the refusals of the
command line - a faulty group file, -G without -t, -G with a switch it does not go with - each of which ends the run
before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import group_ref

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
MAPS = [[0, 1, 1, 2, 3], [0, 4, 0]]  # {t0, t5, t7}, {t1, t2}, singletons


def test_the_reference_folds_members_into_their_group():
    p0 = pairs([(0, 0, -10.0, 2), (0, 1, -7.0, 1), (0, 2, -9.0, 3), (1, 4, -3.0, 1)])
    p1 = pairs([(0, 0, -12.0, 5), (0, 2, -11.0, 1), (1, 1, -1.0, 4)])
    got = group_ref.fold({0: p0, 1: p1}, MAPS, 5)
    rows = [(int(r["query"]), int(r["group"]), int(r["page"]), int(r["db_id"]), float(r["e_min"]), int(r["members"]), int(r["group_hits"]),
             int(r["hits"]), int(r["rank"])) for r in got]
    assert rows == [(0, 0, 1, 0, -12.0, 3, 8, 5, 0),  # t5 beats t0 and t7; hits 2 + 5 + 1, the record's own hits 5
                    (0, 1, 0, 2, -9.0, 2, 4, 3, 0),
                    (1, 3, 0, 4, -3.0, 1, 1, 1, 0),
                    (1, 4, 1, 1, -1.0, 1, 4, 4, 0)]
    # the record is the best member's, field for field
    assert got[0].tobytes()[:p1.dtype.itemsize] == p1[0].tobytes()


def test_the_reference_breaks_ties_by_page_then_db_id_and_takes_the_zeros_as_equal():
    p0 = pairs([(0, 2, -5.0, 1), (0, 1, -5.0, 1), (1, 0, 0.0, 1)])
    p1 = pairs([(0, 0, -5.0, 1), (1, 0, -0.0, 1), (1, 2, -0.0, 1)])
    maps = [[0, 0, 0, 1, 1], [0, 0, 0]]
    got = group_ref.fold({1: p1, 0: p0}, maps, 2)
    assert [(int(r["query"]), int(r["page"]), int(r["db_id"]), int(r["members"])) for r in got] == [(0, 0, 1, 3), (1, 0, 0, 3)]
    assert not np.signbit(got[1]["e_min"])  # page 0's +0.0 wins the tie, with its own bits
    got = group_ref.fold({0: pairs([(1, 0, -0.0, 1)]), 1: pairs([(1, 0, 0.0, 1)])}, maps, 2)
    assert np.signbit(got[0]["e_min"]) and int(got[0]["page"]) == 0


def test_the_reference_ranks_groups_by_the_best_members_key():
    p0 = pairs([(0, 0, -4.0, 1), (0, 1, -6.0, 1), (0, 3, -6.0, 1), (0, 4, -2.0, 1), (2, 4, -1.0, 1)])
    got = group_ref.fold({0: p0}, MAPS, 5, n=3)
    assert [(int(r["query"]), int(r["group"]), int(r["rank"])) for r in got] == [(0, 1, 0), (0, 2, 1), (0, 0, 2), (2, 3, 0)]
    assert len(group_ref.fold({0: p0}, MAPS, 5, n=9)) == 5


def test_the_reference_folds_text_lines():
    lines = ["0,qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ", "1,qa,30,t1,40,1,-12,-12,1,-13,(1-5:9-3) ", "2,qa,30,t2,40,4,-12,-30,1,-13,(2-6:9-3) ",
             "3,qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) "]
    targets = ["t0", "t1", "t2", "t3"]
    got = group_ref.fold_lines(lines, targets, {"t1": "g", "t2": "g"})
    assert got == ["qa,30,t0,40,2,-10,-15,1,-11,(1-5:9-3) ,t0,1,1,2", "qa,30,t1,40,1,-12,-12,1,-13,(1-5:9-3) ,g,2,2,5",
                   "qb,20,t2,40,1,-3,-3,1,-4,(1-5:9-3) ,g,1,2,1"]
    assert group_ref.fold_lines(lines, targets, {"t1": "g", "t2": "g"}, n=1) == [got[1], got[2]]


# ------------------------------------------------------------------------- refusals (no GPU)
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


REFUSALS = {
    "no_tab": ("mdb1 geneA\n", "Error: group file line 1: expected target name, one tab, group name"),
    "two_tabs": ("# a comment\n\nmdb1\tgeneA\nmdb2\tgeneA\textra\n", "Error: group file line 4: expected target name, one tab, group name"),
    "empty_group": ("mdb1\tgeneA\r\nmdb2\t\r\n", "Error: group file line 2: the group name is empty"),
    "unknown_target": ("mdb1\tgeneA\nmdb99\tgeneA\n", 'Error: group file line 2: no database sequence is named "mdb99"'),
    "two_groups": ("mdb1\tgeneA\nmdb2\tgeneB\nmdb1\tgeneA\nmdb1\tgeneB\n",
                   'Error: group file line 4: "mdb1" is listed with the groups "geneA" and "geneB"'),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_a_faulty_group_file_is_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    text, want = REFUSALS[case]
    (tmp_path / "groups.tsv").write_bytes(text.encode())
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-G", str(tmp_path / "groups.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_an_unreadable_group_file_is_refused(tmp_path, golden_dir):
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-G", str(tmp_path / "missing.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == "Error: can't open the group file (-G): " + str(tmp_path / "missing.tsv")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


G = "-G (one line per query-group pair)"
SWITCHES = {
    "without_t": ([], "Error: " + G + " needs -t (per-pair summary lines)"),
    "z": (["-t", "-z", "4"], "Error: " + G + " can't be combined with -z (an empirical p-value per pair from N shuffled decoys)"),
    "k": (["-k", "3"], "Error: " + G + " can't be combined with -k (the N best interaction sites per query)"),
    "q": (["-q"], "Error: " + G + " can't be combined with -q (per-position profile lines)"),
    "r": (["-r", "3"], "Error: " + G + " can't be combined with -r (the N best queries per target)"),
    "c": (["-c", "2"], "Error: " + G + " can't be combined with -c (the regions of each target bound by at least D queries)"),
    "b": (["-b"], "Error: " + G + " can't be combined with -b (binary hit records)"),
}


@pytest.mark.parametrize("case", list(SWITCHES))
def test_switch_combinations_are_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    extra, want = SWITCHES[case]
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra + ["-G", str(tmp_path / "groups.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_one_process_per_gpu_is_refused(tmp_path, golden_dir):
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-G", str(tmp_path / "groups.tsv")], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0].startswith("Error: " + G + " is not supported with one process per GPU (WORLD_SIZE > 1)")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-G STR" in text and "target name, a tab, group name" in text and "not implemented" in text
