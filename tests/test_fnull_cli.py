"""`ris -t -A FILE -F N [-Z SEED]` on the GPU.  The decoys of the queries are written as a FASTA file from
tests/shuffle_ref.py and searched with the existing `ris -t -A`, like the queries themselves; tests/fnull_ref.py folds the
two runs' lines into the lines a -F run has to write.  Lines are compared without their Id; the refusals are in
test_fnull_host.py.

The annotation is the one of test_feature_cli.py (feature_ref.golden_annotation, rebuilt here) with the three consecutive
thirds of every target behind it.  The golden one has seven features on four targets, made from the real hits' own
coordinates; whether decoys meet them was not tried.  With the thirds, N = 4 and seed 7, the plain run has 45 lines: 13 with
NullLE >= 1, 5 with NullHits > 0 and NullLE = 0, and 27 with NullHits = 0 - the three kinds that
test_lines_equal_the_fold_of_the_plain_runs asks for."""
import os
import subprocess

import pytest

import feature_ref
import fnull_ref
import refdump
import shuffle_ref
from test_fnull_host import clean_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
ND, SEED = 4, 7

A_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, Inside")
F_HEADER = A_HEADER + ", Decoys, Null Hits, Null LE, Null Minimum Energy, P Value"


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the annotation as a file; the queries' decoys as a FASTA file; a pair list for the queries and the same for their decoys"""
    tmp = tmp_path_factory.mktemp("fnull_cli")
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        annot = feature_ref.golden_annotation(f.read().splitlines()[2:])
    tnames, tseqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    for t, s in zip(tnames, tseqs):
        annot += [(t, k * len(s) // 3, (k + 1) * len(s) // 3 - 1, f"third{k}") for k in range(3)]
    (tmp / "features.tsv").write_text("".join(f"{t}\t{s}\t{e}\t{n}\n" for t, s, e, n in annot))
    names, seqs = refdump.read_fasta(QUERIES)
    decoy_of = {}
    with open(tmp / "decoys.fa", "w") as f:
        for pos, (name, s) in enumerate(zip(names, seqs)):
            for d in range(ND):
                decoy_of[f"{name}__d{d}"] = (name, d)
                f.write(f">{name}__d{d}\n{shuffle_ref.shuffle(s.encode('latin-1'), SEED, pos, d).decode('latin-1')}\n")
    every = "".join(f"*\t{t}\n" for t in tnames[::2])
    (tmp / "pairs.tsv").write_text(every + f"mq1\t{tnames[1]}\n")
    (tmp / "decoy_pairs.tsv").write_text(every + "".join(f"mq1__d{d}\t{tnames[1]}\n" for d in range(ND)))
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), features=str(tmp / "features.tsv"), decoys=str(tmp / "decoys.fa"),
                decoy_of=decoy_of, pairs=str(tmp / "pairs.tsv"), decoy_pairs=str(tmp / "decoy_pairs.tsv"), cache={})


def ris(case, out, extra, queries=QUERIES, **env):
    """-> (the three header lines, the result lines, the bytes) of the run; a run is made once"""
    from priblast_amd import capi
    key = (tuple(extra), queries, tuple(sorted(env.items())))
    if key not in case["cache"]:
        r = subprocess.run([capi.BIN_PATH, "ris", "-i", queries, "-o", str(case["tmp"] / out), "-d", case["db"]] + extra,
                           capture_output=True, text=True, env=clean_env(**env))
        assert r.returncode == 0, r.stderr
        raw = (case["tmp"] / out).read_bytes()
        lines = raw.decode().splitlines()
        case["cache"][key] = (lines[:3], lines[3:], raw)
    return case["cache"][key]


def f_args(case, extra=()):
    return ["-t", "-A", case["features"], "-F", str(ND), "-Z", str(SEED)] + list(extra)


def assert_null_lines(case, name, extra, decoy_extra):
    """the -F run of `extra` against the fold of the `-t -A` runs of the queries and of their decoys; -> its lines"""
    a = ["-t", "-A", case["features"]]
    _, real, _ = ris(case, name + "_a", a + extra)
    _, decoy, _ = ris(case, name + "_d", a + decoy_extra, queries=case["decoys"])
    head, got, _ = ris(case, name + "_f", f_args(case, extra))
    want = fnull_ref.fold_lines(real, decoy, case["decoy_of"], ND)
    assert head[2] == F_HEADER
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines
    assert [l.split(",", 1)[1] for l in got] == want and len(want) > 3, name
    assert [l.rsplit(",", 5)[0] for l in got] == real  # the columns in front are the -A run's
    return got


def test_lines_equal_the_fold_of_the_plain_runs(case):
    got = assert_null_lines(case, "plain", [], [])
    cols = [l.split(",") for l in got]
    kinds = dict(le=sum(int(c[-3]) >= 1 for c in cols), hits_only=sum(int(c[-4]) > 0 and int(c[-3]) == 0 for c in cols),
                 none=sum(int(c[-4]) == 0 for c in cols))
    print(len(cols), kinds)
    assert all(v >= 1 for v in kinds.values()), kinds  # no comparison of empty nulls
    assert all(int(c[-5]) == ND and 0 <= int(c[-3]) <= int(c[-4]) <= ND for c in cols)
    assert all((c[-2] == "NA") == (int(c[-4]) == 0) for c in cols)
    # -s has no effect
    assert ris(case, "plain_s1", f_args(case, ["-s", "1"]))[1] == got


def test_the_selections_and_a_pair_list(case):
    assert_null_lines(case, "distinct", ["-u"], ["-u"])
    assert_null_lines(case, "chain", ["-j"], ["-j"])
    got = assert_null_lines(case, "listed", ["-L", case["pairs"]], ["-L", case["decoy_pairs"]])
    assert any(int(l.split(",")[-4]) > 0 for l in got)
    args = f_args(case, ["-L", case["pairs"]])
    assert ris(case, "listed_nomask", args, PRB_NULL_MASK="0")[2] == ris(case, "listed_f", args)[2]


SAME_BYTES = {"batch1": dict(PRB_BATCH="1"), "batch2": dict(PRB_BATCH="2"), "nomask": dict(PRB_NULL_MASK="0"),
              "two": dict(PRB_DEVICES="0,0", PRB_BATCH="2"), "split": dict(PRB_DEVICES="0,0", PRB_SPLIT="pages", PRB_BATCH="4")}


@pytest.mark.parametrize("name", list(SAME_BYTES))
def test_the_same_bytes_without_the_mask_in_small_batches_and_with_two_workers(case, name):
    want = ris(case, "plain_f", f_args(case))[2]
    assert want.count(b"\n") > 6
    assert ris(case, name, f_args(case), **SAME_BYTES[name])[2] == want
