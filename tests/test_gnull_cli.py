"""`ris -t -G FILE -P N [-Z SEED]` on the GPU.  The decoys of the queries are written as a FASTA file from
tests/shuffle_ref.py and searched with the existing `ris -t`, like the queries themselves; tests/gnull_ref.py folds the
two runs' lines into the lines a -P run has to write.  Lines are compared without their Id; the refusals are in
test_gnull_host.py."""
import os
import subprocess

import pytest

import gnull_ref
import refdump
import shuffle_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
ND, SEED = 4, 7

G_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Group, Members, Group Size, Group Hits")
P_HEADER = G_HEADER + ", Decoys, Null Hits, Null LE, Null Minimum Energy, P Value"


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the targets in database order; the group file of tests/test_group_cli.py (four consecutive targets to a gene, the
    last five unlisted); the queries' decoys as a FASTA file; a pair list for the queries and the same for their decoys"""
    tmp = tmp_path_factory.mktemp("gnull_cli")
    with open(os.path.join(GOLDEN, "mix_db.fa")) as f:
        targets = [l[1:].strip() for l in f if l.startswith(">")]
    group_of = {t: f"gene{i // 4}" for i, t in enumerate(targets[:-5])}
    text = "# target\tgene\r\n\r\n" + "".join(f"{t}\t{g}\r\n" for t, g in group_of.items()) + f"{targets[0]}\t{group_of[targets[0]]}\n"
    (tmp / "genes.tsv").write_bytes(text.encode())
    (tmp / "own.tsv").write_text("# every target is a group of its own\n")
    names, seqs = refdump.read_fasta(QUERIES)
    decoy_of = {}
    with open(tmp / "decoys.fa", "w") as f:
        for pos, (name, s) in enumerate(zip(names, seqs)):
            for d in range(ND):
                decoy_of[f"{name}__d{d}"] = (name, d)
                f.write(f">{name}__d{d}\n{shuffle_ref.shuffle(s.encode('latin-1'), SEED, pos, d).decode('latin-1')}\n")
    every = "".join(f"*\t{t}\n" for t in targets[::2])
    (tmp / "pairs.tsv").write_text(every + f"mq1\t{targets[1]}\n")
    (tmp / "decoy_pairs.tsv").write_text(every + "".join(f"mq1__d{d}\t{targets[1]}\n" for d in range(ND)))
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), targets=targets, group_of=group_of, genes=str(tmp / "genes.tsv"),
                own=str(tmp / "own.tsv"), decoys=str(tmp / "decoys.fa"), decoy_of=decoy_of, pairs=str(tmp / "pairs.tsv"),
                decoy_pairs=str(tmp / "decoy_pairs.tsv"), cache={})


def ris(case, out, extra, queries=QUERIES, db=None, **env):
    """-> (the three header lines, the result lines, the bytes) of the run; a run without environment changes is made once"""
    from priblast_amd import capi
    key = (tuple(extra), queries, db, tuple(sorted(env.items())))
    if key not in case["cache"]:
        r = subprocess.run([capi.BIN_PATH, "ris", "-i", queries, "-o", str(case["tmp"] / out), "-d", db or case["db"]] + extra,
                           capture_output=True, text=True, env=clean_env(**env))
        assert r.returncode == 0, r.stderr
        raw = (case["tmp"] / out).read_bytes()
        lines = raw.decode().splitlines()
        case["cache"][key] = (lines[:3], lines[3:], raw)
    return case["cache"][key]


def p_args(case, extra=(), genes=None):
    return ["-t", "-G", genes or case["genes"], "-P", str(ND), "-Z", str(SEED)] + list(extra)


def assert_null_lines(case, name, extra, decoy_extra, n=0):
    """the -P run of `extra` against the fold of the `-t` runs of the queries and of their decoys; -> its lines"""
    top = ["-n", str(n)] if n else []
    _, real, _ = ris(case, name + "_t", ["-t"] + extra)
    _, decoy, _ = ris(case, name + "_d", ["-t"] + decoy_extra, queries=case["decoys"])
    head, got, _ = ris(case, name + "_p", p_args(case, extra + top))
    want = gnull_ref.fold_lines(real, decoy, case["decoy_of"], case["targets"], case["group_of"], ND, n)
    assert head[2] == P_HEADER
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines
    assert [l.split(",", 1)[1] for l in got] == want and len(want) > 3, name
    # the columns in front are the -G run's
    _, plain, _ = ris(case, name + "_g", ["-t", "-G", case["genes"]] + extra + top)
    assert [l.rsplit(",", 5)[0] for l in got] == plain
    return got


@pytest.mark.parametrize("n", [0, 3])
def test_lines_equal_the_fold_of_the_plain_runs(case, n):
    got = assert_null_lines(case, f"plain{n}", [], [], n)
    cols = [l.split(",") for l in got]
    assert any(int(c[-4]) > 0 for c in cols)      # NullHits: no comparison of empty nulls
    assert any(int(c[-8]) > 1 for c in cols)      # Members: a group with several members hit
    assert all(int(c[-5]) == ND and 0 <= int(c[-3]) <= int(c[-4]) <= ND for c in cols)
    if n:
        per_query = {}
        for c in cols:
            per_query[c[1]] = per_query.get(c[1], 0) + 1
        assert max(per_query.values()) == n


def test_every_target_a_group_of_its_own_gives_the_pair_level_null(case):
    """ties the new path to `-t -z`: the five null columns, pair for pair"""
    _, got, _ = ris(case, "own_p", p_args(case, genes=case["own"]))
    _, pair, _ = ris(case, "own_z", ["-t", "-z", str(ND), "-Z", str(SEED)])
    key = lambda l: tuple(l.split(",")[1:5:2])
    assert len(got) == len(pair) > 3 and [key(l) for l in got] == [key(l) for l in pair]
    assert [l.rsplit(",", 5)[1:] for l in got] == [l.rsplit(",", 5)[1:] for l in pair]
    assert any(int(l.rsplit(",", 5)[2]) > 0 for l in got)


SAME_BYTES = {"nomask": ([], dict(PRB_NULL_MASK="0")), "batch2": ([], dict(PRB_BATCH="2")), "nomask_n3": (["-n", "3"], dict(PRB_NULL_MASK="0")),
              "split_n3": (["-n", "3"], dict(PRB_DEVICES="0,0", PRB_SPLIT="pages", PRB_BATCH="4"))}


@pytest.mark.parametrize("name", list(SAME_BYTES))
def test_the_same_bytes_without_the_mask_and_in_small_batches(case, name):
    extra, env = SAME_BYTES[name]
    want = ris(case, "base" + "".join(extra), p_args(case, extra))[2]
    assert want.count(b"\n") > 6
    assert ris(case, name, p_args(case, extra), **env)[2] == want


def test_under_a_pair_list(case):
    got = assert_null_lines(case, "listed", ["-L", case["pairs"]], ["-L", case["decoy_pairs"]], n=2)
    assert any(int(l.split(",")[-4]) > 0 for l in got)
    args = p_args(case, ["-L", case["pairs"], "-n", "2"])
    assert ris(case, "listed_nomask", args, PRB_NULL_MASK="0")[2] == ris(case, "listed_p", args)[2]


def test_the_same_lines_on_other_pages(case):
    """the same database cut into more pages (`db -c`): other page borders within the groups"""
    from priblast_amd import capi
    db = str(case["tmp"] / "db4")
    subprocess.run([capi.BIN_PATH, "db", "-i", os.path.join(GOLDEN, "mix_db.fa"), "-o", db, "-c", "4"], check=True, env=clean_env())
    for extra in ([], ["-n", "3"]):
        _, want, _ = ris(case, "pages_base", p_args(case, extra))
        _, got, _ = ris(case, "pages_db4", p_args(case, extra), db=db)
        assert got == want and len(want) > 3
