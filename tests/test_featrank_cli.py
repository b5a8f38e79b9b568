"""`ris -t -A FILE -B N` on the GPU, on `mix_q.fa` against `mixdb` with the annotation of test_featuretop_cli.py (the
golden annotation with the three consecutive thirds of every target behind it): every line of a -B run, its Id apart, is
a line of the same run without -B; a feature has min(N, its lines there) of them; and their order - by feature in the
order of the annotation file's lines, then rank - is that of the exact records through the C ABI (tests/featrank_ref.py
pins those in test_gpu_featrank.py), not of the printed energies, which can hide a tie.  The bytes do not depend on
PRB_BATCH, on two workers, nor on PRB_SPLIT.  The refusals are in test_featrank_host.py."""
import os
import subprocess

import pytest

import feature_ref
import refdump

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")

A_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, Inside")


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the annotation as a list in the file's order and as a file - no two of its lines alike -, and a pair list"""
    tmp = tmp_path_factory.mktemp("featrank_cli")
    with open(os.path.join(GOLDEN, "mix_ris_s1.out")) as f:
        annot = feature_ref.golden_annotation(f.read().splitlines()[2:])
    tnames, tseqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_db.fa"))
    for t, s in zip(tnames, tseqs):
        annot += [(t, k * len(s) // 3, (k + 1) * len(s) // 3 - 1, f"third{k}") for k in range(3)]
    assert len(set(annot)) == len(annot) and len(set(tnames)) == len(tnames)
    (tmp / "features.tsv").write_text("# features\n\n" + "".join(f"{t}\t{s}\t{e}\t{n}\n" for t, s, e, n in annot))
    (tmp / "pairs.tsv").write_text("".join(f"*\t{t}\n" for t in tnames[::2]))
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), annot=annot, targets=tnames, features=str(tmp / "features.tsv"),
                pairs=str(tmp / "pairs.tsv"))


def ris(case, out, extra, **env):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(case["tmp"] / out), "-d", case["db"]] + extra, capture_output=True,
                       text=True, env=clean_env(**env))
    assert r.returncode == 0, r.stderr
    lines = (case["tmp"] / out).read_text().splitlines()
    return lines[:3], lines[3:], r.stderr


def no_id(lines):
    return [l.split(",", 1)[1] for l in lines]


def feature_of(line):
    """(target name, feature name, feature range) of a line: what names a feature of this annotation"""
    cols = line.split(",")
    return cols[3], cols[-3], cols[-2]


def expected_order(case, n, **opts):
    """(query name, target name, feature name, feature range) of the kept records by feature and rank, from the exact records"""
    from priblast_amd import capi
    qnames, seqs = refdump.read_fasta(QUERIES)
    with capi.Context(0) as ctx:
        db = capi.Db(ctx, case["db"])
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        where = {db.seq_name(p, i): (p, i) for p in range(db.npages) for i in range(db.page_info(p)[0])}
        with capi.Annotation(ctx, db, [where[t] + (s, e) for t, s, e, _ in case["annot"]]) as an:
            recs, _ = capi.search_featrank(ctx, db, an, n, [(qb, list(range(len(seqs))))], opts=capi.default_opts(**opts))
        out = []
        for r in recs:
            t, s, e, name = case["annot"][int(r["feature"])]
            assert db.seq_name(int(r["page"]), int(r["db_id"])) == t
            out.append((qnames[int(r["query"])], t, name, f"{s}-{e}"))
        assert [(int(r["feature"]), int(r["rank"])) for r in recs] == sorted((int(r["feature"]), int(r["rank"])) for r in recs)
        qb.close()
        db.close()
    return out


def assert_rank_lines(case, name, extra, n=2, **opts):
    """the -B run of `extra` against the run without -B and the exact records; -> the -B run's file name"""
    head, got, _ = ris(case, name + "_b", ["-t", "-A", case["features"], "-B", str(n)] + extra)
    head_a, plain, _ = ris(case, name + "_a", ["-t", "-A", case["features"]] + extra)
    assert head == head_a and head[2] == A_HEADER and len(got) > 3
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines, from 0
    assert set(no_id(got)) <= set(no_id(plain)) and len(set(got)) == len(got)
    for f in set(feature_of(l) for l in plain):  # (a feature that no query touches has no line in either run)
        assert sum(feature_of(l) == f for l in got) == min(n, sum(feature_of(l) == f for l in plain)), f
    assert [(l.split(",")[1],) + feature_of(l) for l in got] == expected_order(case, n, **opts)
    return name + "_b"


@pytest.fixture(scope="module")
def base(case):
    """the -B 2 run of the default options, checked against the run without -B and the exact records: its bytes"""
    return (case["tmp"] / assert_rank_lines(case, "plain", [])).read_bytes()


def test_rank_lines_are_feature_lines_in_the_order_of_the_exact_records(case, base):
    _, plain, _ = ris(case, "plain_a", ["-t", "-A", case["features"]])
    assert base.count(b"\n") - 3 < len(plain)  # (-B 2 cuts something)
    # -s has no effect
    ris(case, "s1", ["-t", "-A", case["features"], "-B", "2", "-s", "1"])
    assert (case["tmp"] / "s1").read_bytes() == base


# one query per batch; two workers on one GPU that share out the batches, and that share the pages of every batch
SAME_BYTES = {"batch1": dict(PRB_BATCH="1"), "two": dict(PRB_DEVICES="0,0", PRB_BATCH="2"), "split": dict(PRB_DEVICES="0,0", PRB_SPLIT="pages"),
              "split_batch3": dict(PRB_DEVICES="0,0", PRB_SPLIT="pages", PRB_BATCH="3")}


@pytest.mark.parametrize("name", list(SAME_BYTES))
def test_small_batches_and_two_workers_write_the_same_bytes(case, base, name):
    env = SAME_BYTES[name]
    _, _, err = ris(case, name, ["-t", "-A", case["features"], "-B", "2"], **env)
    assert (case["tmp"] / name).read_bytes() == base
    assert ("page split:" in err) == ("PRB_SPLIT" in env)


def test_rank_lines_of_one_query_per_feature(case):
    assert_rank_lines(case, "best", [], n=1)


@pytest.mark.parametrize("switch", ["-u", "-j"])
def test_rank_lines_of_the_distinct_sites_and_of_the_chains(case, switch):
    assert_rank_lines(case, "distinct" if switch == "-u" else "chain", [switch], **{("distinct" if switch == "-u" else "chain") + "_sites": 1})


def test_rank_lines_of_listed_pairs(case):
    """-L: against the filtered -t -A lines (the exact records of a masked search are the other tables' tests')"""
    _, got, _ = ris(case, "listed_b", ["-t", "-A", case["features"], "-B", "2", "-L", case["pairs"]])
    _, plain, _ = ris(case, "listed_a", ["-t", "-A", case["features"], "-L", case["pairs"]])
    assert set(no_id(got)) <= set(no_id(plain)) and 0 < len(got) <= len(plain)
    assert all(l.split(",")[3] in case["targets"][::2] for l in got)
    for f in set(feature_of(l) for l in plain):
        assert sum(feature_of(l) == f for l in got) == min(2, sum(feature_of(l) == f for l in plain)), f
