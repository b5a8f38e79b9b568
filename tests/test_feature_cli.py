"""`ris -t -A FILE` on the GPU: the lines of an -A run are the reference fold (tests/feature_ref.py) of the `-s 1` lines that
the same run writes without -t -A - with -u, -j and -L, with small batches, with two workers, and with two workers that
share the pages of the batch, which must write the same bytes.  Lines are compared without their Id (an -A run numbers its
own lines) and field by field as text, but for the summed energy (feature_ref.same_lines says why and how closely).  The
refusals of the switch row and of faulty annotation files are those of test_feature_host.py, run here beside the GPU."""
import os
import subprocess

import pytest

import feature_ref
import test_feature_host as host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")

A_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, Inside")


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the golden annotation of `mix` as a file (CRLF, a comment, an empty line), and a pair list"""
    tmp = tmp_path_factory.mktemp("feature_cli")
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        annot = feature_ref.golden_annotation(f.read().splitlines()[2:])
    text = "# target\tstart\tend\tname\r\n\r\n" + "".join(f"{t}\t{s}\t{e}\t{n}\r\n" for t, s, e, n in annot)
    (tmp / "features.tsv").write_bytes(text.encode())
    annot_of = {}
    for t, s, e, n in annot:
        annot_of.setdefault(t, []).append((s, e, n))
    with open(os.path.join(GOLDEN, "mix_db.fa")) as f:
        targets = [l[1:].strip() for l in f if l.startswith(">")]
    (tmp / "pairs.tsv").write_text("".join(f"*\t{t}\n" for t in targets[::2]) + f"mq0\t{annot[2][0]}\n")
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), annot_of=annot_of, features=str(tmp / "features.tsv"), pairs=str(tmp / "pairs.tsv"))


def ris(case, out, extra, **env):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(case["tmp"] / out), "-d", case["db"]] + extra, capture_output=True,
                       text=True, env=host.clean_env(**env))
    assert r.returncode == 0, r.stderr
    with open(case["tmp"] / out) as f:
        lines = f.read().splitlines()
    return lines[:3], lines[3:], r.stderr


def assert_feature_lines(case, name, extra, **env):
    """the -t -A run of `extra` against the fold of the -s 1 run of `extra`; -> the -A run's (header, lines)"""
    _, full, _ = ris(case, name + "_s1", ["-s", "1"] + extra, **env)
    head, got, _ = ris(case, name + "_a", ["-t", "-A", case["features"]] + extra, **env)
    want, _ = feature_ref.fold_lines(full, case["annot_of"])
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines
    assert feature_ref.same_lines(got, want) and len(want) > 3, (name, got, want)
    return head, got


def test_feature_lines_and_header(case):
    head, got = assert_feature_lines(case, "plain", [])
    assert head[2] == A_HEADER
    names = {l.split(",")[11] for l in got}
    assert {"left", "right", "nested", "outer"} <= names and "away" not in names
    # -s has no effect
    assert ris(case, "plain_s1", ["-t", "-s", "1", "-A", case["features"]])[1] == got


def test_feature_lines_of_the_distinct_sites_the_chain_and_of_listed_pairs(case):
    assert_feature_lines(case, "distinct", ["-u"])
    assert_feature_lines(case, "chain", ["-j"])
    assert_feature_lines(case, "listed", ["-L", case["pairs"]])


def test_small_batches_and_two_workers_write_the_same_bytes(case):
    args = ["-t", "-A", case["features"]]
    one = ris(case, "one", args, PRB_DEVICES="0")
    assert len(one[1]) > 3
    for name, env in (("batch1", dict(PRB_BATCH="1")), ("two", dict(PRB_DEVICES="0,0")), ("split", dict(PRB_DEVICES="0,0", PRB_SPLIT="pages"))):
        other = ris(case, name, args, **env)
        assert ("page split:" in other[2]) == (name == "split")
        assert (case["tmp"] / "one").read_bytes() == (case["tmp"] / name).read_bytes(), name


@pytest.mark.parametrize("which", list(host.SWITCHES))
def test_every_refusal_of_the_switch_row(tmp_path, golden_dir, which):
    host.check_switch_refusal(tmp_path, golden_dir, which)


@pytest.mark.parametrize("which", list(host.FILES))
def test_bad_annotation_files_are_refused_with_line_numbers(tmp_path, golden_dir, which):
    host.check_file_refusal(tmp_path, golden_dir, which)
