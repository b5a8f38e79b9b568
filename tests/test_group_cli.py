"""`ris -t -G FILE` on the GPU: the lines of a -G run are the reference fold (tests/group_ref.py) of the lines that the
same run writes without -G - with -n N, with -u, with -L, and with two workers that share the pages of the batch.  Lines
are compared without their Id (a -G run numbers its own lines); the refusals are in test_group_host.py."""
import os
import subprocess

import pytest

import group_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")

T_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair")
G_HEADER = T_HEADER + ", Group, Members, Group Size, Group Hits"


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the targets in database order, and a group file: four consecutive targets to a gene (CRLF, a comment, an empty
    line, a target twice), the last five targets unlisted"""
    tmp = tmp_path_factory.mktemp("group_cli")
    with open(os.path.join(GOLDEN, "mix_db.fa")) as f:
        targets = [l[1:].strip() for l in f if l.startswith(">")]
    assert len(targets) > 12 and len(set(targets)) == len(targets)
    group_of = {t: f"gene{i // 4}" for i, t in enumerate(targets[:-5])}
    text = "# target\tgene\r\n\r\n" + "".join(f"{t}\t{g}\r\n" for t, g in group_of.items()) + f"{targets[0]}\t{group_of[targets[0]]}\n"
    (tmp / "genes.tsv").write_bytes(text.encode())
    (tmp / "pairs.tsv").write_text("".join(f"*\t{t}\n" for t in targets[::2]) + f"mq1\t{targets[1]}\n")
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), targets=targets, group_of=group_of, genes=str(tmp / "genes.tsv"),
                pairs=str(tmp / "pairs.tsv"))


def ris(case, out, extra, **env):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(case["tmp"] / out), "-d", case["db"]] + extra, capture_output=True,
                       text=True, env=clean_env(**env))
    assert r.returncode == 0, r.stderr
    with open(case["tmp"] / out) as f:
        lines = f.read().splitlines()
    return lines[:3], lines[3:], r.stderr


def assert_group_lines(case, name, extra, n=0, **env):
    """the -G run of `extra` against the fold of the run without -G; -> the -G run's (header, lines)"""
    _, plain, _ = ris(case, name + "_t", ["-t"] + extra, **env)
    head, got, _ = ris(case, name + "_g", ["-t", "-G", case["genes"]] + extra + (["-n", str(n)] if n else []), **env)
    want = group_ref.fold_lines(plain, case["targets"], case["group_of"], n)
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines
    assert [l.split(",", 1)[1] for l in got] == want and len(want) > 3, name
    return head, got


def test_group_lines_and_header(case):
    head, got = assert_group_lines(case, "plain", [])
    assert head[2] == G_HEADER
    t_head, plain, _ = ris(case, "plain_t", ["-t"])
    assert t_head[2] == T_HEADER and t_head[:2] == head[:2] and len(got) < len(plain)
    assert any(int(l.split(",")[-3]) > 1 for l in got)  # a group with several members hit


def test_the_best_groups_of_each_query(case):
    head, got = assert_group_lines(case, "top", [], n=3)
    assert head[2] == G_HEADER
    per_query = {}
    for l in got:
        per_query[l.split(",")[1]] = per_query.get(l.split(",")[1], 0) + 1
    assert max(per_query.values()) == 3


def test_group_lines_of_the_distinct_sites_and_of_listed_pairs(case):
    assert_group_lines(case, "distinct", ["-u"])
    assert_group_lines(case, "listed", ["-L", case["pairs"]], n=2)


def test_small_batches_write_the_same_lines(case):
    assert_group_lines(case, "batch2", [], PRB_BATCH="2")


def test_two_workers_sharing_pages_write_the_same_bytes(case):
    for name, extra in (("split", []), ("split_n", ["-n", "3"])):
        args = ["-t", "-G", case["genes"]] + extra
        one = ris(case, name + "_one", args, PRB_DEVICES="0")
        two = ris(case, name + "_two", args, PRB_DEVICES="0,0", PRB_SPLIT="pages")
        assert "page split:" in two[2] and "page split" not in one[2]
        assert (case["tmp"] / (name + "_one")).read_bytes() == (case["tmp"] / (name + "_two")).read_bytes() and len(one[1]) > 3
