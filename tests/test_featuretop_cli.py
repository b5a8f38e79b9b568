"""`ris -t -A FILE -N K` on the GPU, on `mix_q.fa` against `mixdb` with K = 2.  The exact order of the ranked cut is pinned on
doubles in test_gpu_featuretop_kernel.py; here the lines of an -N run are checked against the lines of the `-t -A` run of the
same options (featuretop_ref.select_lines): every line is one of them, Ids count the written lines, a query has min(K, its
lines), printed minimum energies do not decrease with rank and no dropped line prints a lower one than the last kept - with
-u, -j and -L, and with the same bytes in small batches, with two workers, and with two workers that share the pages.  With
-F the lines are lines of the `-F` run, with and without the decoys' mask.  The refusals are in test_featuretop_host.py.

The annotation is the one of test_fnull_cli.py: feature_ref.golden_annotation with the three consecutive thirds of every
target behind it, so that a query has several lines and decoys meet features."""
import os
import subprocess

import pytest

import feature_ref
import featuretop_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
K, ND, SEED = 2, 4, 7

A_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, Inside")
F_HEADER = A_HEADER + ", Decoys, Null Hits, Null LE, Null Minimum Energy, P Value"


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the annotation as a file and a pair list; a run is made once"""
    tmp = tmp_path_factory.mktemp("featuretop_cli")
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        annot = feature_ref.golden_annotation(f.read().splitlines()[2:])
    tnames, tseqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    for t, s in zip(tnames, tseqs):
        annot += [(t, k * len(s) // 3, (k + 1) * len(s) // 3 - 1, f"third{k}") for k in range(3)]
    (tmp / "features.tsv").write_text("".join(f"{t}\t{s}\t{e}\t{n}\n" for t, s, e, n in annot))
    (tmp / "pairs.tsv").write_text("".join(f"*\t{t}\n" for t in tnames[::2]) + f"mq1\t{tnames[1]}\n")
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), features=str(tmp / "features.tsv"), pairs=str(tmp / "pairs.tsv"), cache={})


def ris(case, out, extra, **env):
    """-> (the three header lines, the result lines, the bytes) of the run"""
    from priblast_amd import capi
    key = (tuple(extra), tuple(sorted(env.items())))
    if key not in case["cache"]:
        r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(case["tmp"] / out), "-d", case["db"]] + extra,
                           capture_output=True, text=True, env=clean_env(**env))
        assert r.returncode == 0, r.stderr
        raw = (case["tmp"] / out).read_bytes()
        lines = raw.decode().splitlines()
        case["cache"][key] = (lines[:3], lines[3:], raw)
    return case["cache"][key]


def a_args(case, extra=()):
    return ["-t", "-A", case["features"]] + list(extra)


def assert_ranked_cut(case, name, extra):
    head, full, _ = ris(case, name + "_a", a_args(case, extra))
    head_n, got, _ = ris(case, name + "_n", a_args(case, extra) + ["-N", str(K)])
    assert head_n == head and head[2] == A_HEADER  # no new column
    assert featuretop_ref.select_lines(got, full, K) is None, (name, got, full)
    assert 3 < len(got) < len(full), name  # something is kept, and something cut
    return got, full


def test_the_lines_are_a_ranked_cut_of_the_plain_run(case):
    got, full = assert_ranked_cut(case, "plain", [])
    per_query = {}
    for l in full:
        per_query[l.split(",")[1]] = per_query.get(l.split(",")[1], 0) + 1
    assert max(per_query.values()) > K and len(per_query) > 1
    # -s has no effect; K beyond every query's lines keeps them all, by rank
    assert ris(case, "plain_s1", a_args(case, ["-s", "1", "-N", str(K)]))[1] == got
    every = ris(case, "plain_all", a_args(case, ["-N", "1024"]))[1]
    assert featuretop_ref.select_lines(every, full, 1024) is None and len(every) == len(full)


def test_with_the_selections_and_a_pair_list(case):
    assert_ranked_cut(case, "distinct", ["-u"])
    assert_ranked_cut(case, "chain", ["-j"])
    assert_ranked_cut(case, "listed", ["-L", case["pairs"]])


SAME_BYTES = {"batch1": dict(PRB_BATCH="1"), "two": dict(PRB_DEVICES="0,0"), "split": dict(PRB_DEVICES="0,0", PRB_SPLIT="pages")}


@pytest.mark.parametrize("name", list(SAME_BYTES))
def test_small_batches_and_two_workers_write_the_same_bytes(case, name):
    args = a_args(case, ["-N", str(K)])
    want = ris(case, "one", args, PRB_DEVICES="0")[2]
    assert want.count(b"\n") > 6
    assert ris(case, name, args, **SAME_BYTES[name])[2] == want


def test_with_decoys_the_lines_are_lines_of_the_uncut_null_run(case):
    f = a_args(case, ["-F", str(ND), "-Z", str(SEED)])
    head, full, _ = ris(case, "f_full", f)
    head_n, got, raw = ris(case, "f_cut", f + ["-N", str(K)])
    assert head_n == head and head[2] == F_HEADER
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines
    stripped = [l.split(",", 1)[1] for l in full]
    assert all(l.split(",", 1)[1] in stripped for l in got) and 3 < len(got) < len(full)  # the null columns are the uncut run's
    # ... and in front of them stand the lines of the -N run without decoys, in its order
    assert [l.rsplit(",", 5)[0] for l in got] == ris(case, "f_plain_n", a_args(case, ["-N", str(K)]))[1]
    assert ris(case, "f_cut_nomask", f + ["-N", str(K)], PRB_NULL_MASK="0")[2] == raw
