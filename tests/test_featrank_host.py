"""`ris -t -A FILE -B N` without a GPU: the yardstick (tests/featrank_ref.py) on a hand-made array, the refusals of the
command line - -B without -A, with -F or -N, a value out of range, what -A does not go with in -A's words, an annotation
without features - each of which ends the run before any GPU work, and the usage text."""
import os
import subprocess

import numpy as np
import pytest

import featrank_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


# ------------------------------------------------------------------------- the yardstick
def test_rank_groups_by_feature_orders_by_energy_then_identifier_and_cuts():
    from priblast_amd import capi
    rows = [(7, 2, -3.0), (1, 2, -9.0), (4, 0, -9.0), (2, 2, -9.0), (3, 0, 0.0), (9, 0, -0.0), (5, 4, -4.0)]  # (identifier, feature, e_min)
    recs = np.zeros(len(rows), capi.FEATRANK_DTYPE)
    for i, (q, f, e) in enumerate(rows):
        recs[i]["query"], recs[i]["feature"], recs[i]["e_min"], recs[i]["inside"], recs[i]["rank"] = q, f, e, i, 77
    pick = lambda n, parts=(recs,): [(int(r["feature"]), int(r["query"]), int(r["rank"])) for r in featrank_ref.rank(list(parts), n)]
    assert pick(1) == [(0, 4, 0), (2, 1, 0), (4, 5, 0)]                                   # of the tie at -9 the lower identifier
    assert pick(2) == [(0, 4, 0), (0, 3, 1), (2, 1, 0), (2, 2, 1), (4, 5, 0)]             # +0.0 and -0.0 tie: identifier 3 first
    assert pick(1024) == [(0, 4, 0), (0, 3, 1), (0, 9, 2), (2, 1, 0), (2, 2, 1), (2, 7, 2), (4, 5, 0)]
    assert pick(2, (recs[4:], recs[:0], recs[:4])) == pick(2)                             # however the records are cut
    kept = featrank_ref.rank([recs], 2)
    assert kept[3]["inside"] == 3 and bool(np.signbit(featrank_ref.rank([recs], 3)[2]["e_min"]))  # field for field, the bits kept
    assert featrank_ref.rank([recs[:0]], 3) is None and featrank_ref.rank_bytes([], 3) == b""
    plain = np.zeros(2, capi.FEATURE_DTYPE)
    plain["query"], plain["feature"], plain["e_min"] = [1, 0], [3, 5], [-2.0, -1.0]
    got = featrank_ref.with_ids(plain, [40, 50])
    assert got.dtype == capi.FEATRANK_DTYPE and got["query"].tolist() == [50, 40] and got["feature"].tolist() == [3, 5]


# ------------------------------------------------------------------------- the command line
def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, features="mdb1\t3\t9\tcds\n", **env):
    from priblast_amd import capi
    (tmp_path / "features.tsv").write_text(features)
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    extra = [str(tmp_path / "groups.tsv") if x == "GROUPS" else str(tmp_path / "features.tsv") if x == "FEATURES" else x for x in extra]
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / "out"), "-d", db] + extra, capture_output=True, text=True,
                          env=clean_env(**env))


A = "-A (one line per query-feature pair)"
B = "-B (the N best queries per feature)"
RANGE = "Error: -B needs an integer between 1 and 1024 (this build's limit)"
RANK_MODE = " is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
REFUSALS = {
    "without_A": (["-t", "-B", "2"], {}, "Error: " + B + " needs " + A),
    "without_t": (["-A", "FEATURES", "-B", "2"], {}, "Error: " + A + " needs -t (per-pair summary lines)"),
    "F": (["-t", "-A", "FEATURES", "-F", "4", "-B", "2"], {},
          "Error: " + B + " can't be combined with -F (an empirical p-value per query-feature pair from N shuffled decoys)"),
    "N": (["-t", "-A", "FEATURES", "-N", "3", "-B", "2"], {}, "Error: " + B + " can't be combined with -N (the N best features per query)"),
    "zero": (["-t", "-A", "FEATURES", "-B", "0"], {}, RANGE),
    "too_many": (["-t", "-A", "FEATURES", "-B", "1025"], {}, RANGE),
    "not_a_number": (["-t", "-A", "FEATURES", "-B", "two"], {}, RANGE),
    # what -A can't be combined with is refused in -A's words, as without -B
    "G": (["-t", "-G", "GROUPS", "-A", "FEATURES", "-B", "2"], {}, "Error: " + A + " can't be combined with -G (one line per query-group pair)"),
    "r": (["-r", "3", "-A", "FEATURES", "-B", "2"], {}, "Error: " + A + " can't be combined with -r (the N best queries per target)"),
    "r_first": (["-r", "3", "-B", "2", "-t", "-A", "FEATURES"], {}, "Error: " + A + " can't be combined with -r (the N best queries per target)"),
    "k": (["-k", "3", "-A", "FEATURES", "-B", "2"], {}, "Error: " + A + " can't be combined with -k (the N best interaction sites per query)"),
    "b": (["-t", "-b", "-A", "FEATURES", "-B", "2"], {}, "Error: " + A + " can't be combined with -b (binary hit records)"),
    "rank_mode": (["-t", "-A", "FEATURES", "-B", "2"], dict(WORLD_SIZE="2", RANK="0"), "Error: " + A + RANK_MODE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_any_gpu_work(tmp_path, golden_dir, case):
    extra, env, want = REFUSALS[case]
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), extra, **env)
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_an_annotation_without_features_is_refused_before_any_gpu_work(tmp_path, golden_dir):
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-A", "FEATURES", "-B", "2"], features="# nothing\n\n")
    first = (r.stderr.splitlines() or [""])[0]
    assert first.startswith("Error: annotation file ") and first.endswith("has no feature: " + B + " needs one")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-B INT" in text and "per feature" in text and "the best queries per feature: -B" in text
    assert "numbered in the order of the annotation file's lines" in text
