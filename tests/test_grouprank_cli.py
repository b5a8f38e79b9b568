"""`ris -t -G FILE -R N`: the refusals of the command line, each of which ends the run before any GPU work, and - on the
GPU - the lines of a -R run on the `mix` fixture: every line, its Id apart, is a line of the same run without -R; a group
has min(N, its lines there) of them; and their order - by group in database order, then rank - is that of the exact
records through the C ABI (tests/grouprank_ref.py pins those in test_gpu_grouprank.py), not of the printed energies,
which can hide a tie.  The bytes do not depend on PRB_BATCH, on two workers, nor on PRB_SPLIT."""
import os
import subprocess

import numpy as np
import pytest

import refdump

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")

G_HEADER = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
            "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Group, Members, Group Size, Group Hits")
G = "-G (one line per query-group pair)"
R = "-R (the N best queries per group)"
RANGE = "Error: -R needs an integer between 1 and 1024 (this build's limit)"


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        env.pop(k, None)
    env.update(kw)
    return env


def run_ris(out, db, extra, **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(out), "-d", db] + extra, capture_output=True, text=True,
                          env=clean_env(**env))


# ------------------------------------------------------------------------- refusals (no GPU)
REFUSALS = {
    "without_G": (["-t", "-R", "2"], {}, "Error: " + R + " needs " + G),
    "without_t": (["-G", "@", "-R", "2"], {}, "Error: " + G + " needs -t (per-pair summary lines)"),
    "n": (["-t", "-G", "@", "-n", "3", "-R", "2"], {}, "Error: " + R + " can't be combined with -n (the N best pairs per query)"),
    "P": (["-t", "-G", "@", "-P", "4", "-R", "2"], {},
          "Error: " + R + " can't be combined with -P (an empirical p-value per query-group pair from N shuffled decoys)"),
    "zero": (["-t", "-G", "@", "-R", "0"], {}, RANGE),
    "too_many": (["-t", "-G", "@", "-R", "1025"], {}, RANGE),
    "not_a_number": (["-t", "-G", "@", "-R", "two"], {}, RANGE),
    # what -G can't be combined with is refused in -G's words, as without -R
    "r": (["-G", "@", "-r", "3", "-R", "2"], {}, "Error: " + G + " can't be combined with -r (the N best queries per target)"),
    "r_first": (["-r", "3", "-R", "2", "-t", "-G", "@"], {}, "Error: " + G + " can't be combined with -r (the N best queries per target)"),
    "k": (["-G", "@", "-k", "3", "-R", "2"], {}, "Error: " + G + " can't be combined with -k (the N best interaction sites per query)"),
    "b": (["-t", "-G", "@", "-b", "-R", "2"], {}, "Error: " + G + " can't be combined with -b (binary hit records)"),
    "rank_mode": (["-t", "-G", "@", "-R", "2"], dict(WORLD_SIZE="2", RANK="0"),
                  "Error: " + G + " is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_any_gpu_work(tmp_path, golden_dir, case):
    extra, env, want = REFUSALS[case]
    (tmp_path / "groups.tsv").write_text("mdb1\tgeneA\n")
    r = run_ris(tmp_path / "out", os.path.join(golden_dir, "mixdb"), [str(tmp_path / "groups.tsv") if a == "@" else a for a in extra], **env)
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-R INT" in text and "per group" in text and "the best queries per group: -R" in text


# ------------------------------------------------------------------------- parity (GPU)
@pytest.fixture(scope="module")
def case(tmp_path_factory, golden_dir):
    """the targets in database order, and a group file: four consecutive targets to a gene - so genes span the pages'
    borders -, the last five targets unlisted; the groups' indices as -G assigns them (by first member, in database order)"""
    tmp = tmp_path_factory.mktemp("grouprank_cli")
    with open(os.path.join(GOLDEN, "mix_db.fa")) as f:
        targets = [l[1:].strip() for l in f if l.startswith(">")]
    group_of = {t: f"gene{i // 4}" for i, t in enumerate(targets[:-5])}
    (tmp / "genes.tsv").write_text("".join(f"{t}\t{g}\n" for t, g in group_of.items()))
    (tmp / "pairs.tsv").write_text("".join(f"*\t{t}\n" for t in targets[::2]))
    names = []
    for t in targets:
        if group_of.get(t, t) not in names:
            names.append(group_of.get(t, t))
    return dict(tmp=tmp, db=os.path.join(golden_dir, "mixdb"), targets=targets, group_of=group_of, group_names=names, genes=str(tmp / "genes.tsv"),
                pairs=str(tmp / "pairs.tsv"))


def ris(case, out, extra, **env):
    r = run_ris(case["tmp"] / out, case["db"], extra, **env)
    assert r.returncode == 0, r.stderr
    lines = (case["tmp"] / out).read_text().splitlines()
    return lines[:3], lines[3:], r.stderr


def no_id(lines):
    return [l.split(",", 1)[1] for l in lines]


def expected_order(case, n, **opts):
    """(query name, target name, group name) of the kept records by group and rank, from the exact records"""
    from priblast_amd import capi
    qnames, seqs = refdump.read_fasta(QUERIES)
    with capi.Context(0) as ctx:
        db = capi.Db(ctx, case["db"])
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        maps, t = [], 0
        for p in range(db.npages):
            nseq = db.page_info(p)[0]
            maps.append([case["group_names"].index(case["group_of"].get(x, x)) for x in case["targets"][t:t + nseq]])
            t += nseq
        recs = capi.search_grouprank(ctx, db, maps, len(case["group_names"]), n, [(qb, list(range(len(seqs))))], opts=capi.default_opts(**opts))
        out = [(qnames[int(r["query"])], db.seq_name(int(r["page"]), int(r["db_id"])), case["group_names"][int(r["group"])]) for r in recs]
        assert [(int(r["group"]), int(r["rank"])) for r in recs] == sorted((int(r["group"]), int(r["rank"])) for r in recs)
        qb.close()
        db.close()
    return out


def assert_rank_lines(case, name, extra, n=2, **opts):
    """the -R run of `extra` against the run without -R and the exact records; -> the -R run's file name"""
    head, got, _ = ris(case, name + "_r", ["-t", "-G", case["genes"], "-R", str(n)] + extra)
    _, plain, _ = ris(case, name + "_g", ["-t", "-G", case["genes"]] + extra)
    assert head[2] == G_HEADER and len(got) > 3
    assert [l.split(",")[0] for l in got] == [str(k) for k in range(len(got))]  # Id counts the written lines, from 0
    assert set(no_id(got)) <= set(no_id(plain)) and len(set(got)) == len(got)
    group = lambda l: l.split(",")[-4]
    for g in set(group(l) for l in plain):
        assert sum(group(l) == g for l in got) == min(n, sum(group(l) == g for l in plain)), g
    assert [(l.split(",")[1], l.split(",")[3], group(l)) for l in got] == expected_order(case, n, **opts)
    return name + "_r"


@pytest.mark.gpu
def test_rank_lines_are_group_lines_in_the_order_of_the_exact_records(case):
    base = assert_rank_lines(case, "plain", [])
    want = (case["tmp"] / base).read_bytes()
    # one query per batch; two workers on one GPU that share out the batches, and that share the pages of every batch
    for name, env in (("batch1", dict(PRB_BATCH="1")), ("two", dict(PRB_DEVICES="0,0", PRB_BATCH="2")),
                      ("split", dict(PRB_DEVICES="0,0", PRB_SPLIT="pages")), ("split_batch3", dict(PRB_DEVICES="0,0", PRB_SPLIT="pages", PRB_BATCH="3"))):
        _, _, err = ris(case, name, ["-t", "-G", case["genes"], "-R", "2"], **env)
        assert (case["tmp"] / name).read_bytes() == want, name
        assert ("page split:" in err) == ("PRB_SPLIT" in env)


@pytest.mark.gpu
def test_rank_lines_of_one_query_per_group(case):
    assert_rank_lines(case, "best", [], n=1)


@pytest.mark.gpu
def test_rank_lines_of_the_distinct_sites_the_chains_and_of_listed_pairs(case):
    assert_rank_lines(case, "distinct", ["-u"], distinct_sites=1)
    assert_rank_lines(case, "chain", ["-j"], chain_sites=1)
    # -L: against the filtered -t -G lines (the exact records of a masked search are test_gpu_grouprank.py's)
    _, got, _ = ris(case, "listed_r", ["-t", "-G", case["genes"], "-R", "2", "-L", case["pairs"]])
    _, plain, _ = ris(case, "listed_g", ["-t", "-G", case["genes"], "-L", case["pairs"]])
    assert set(no_id(got)) <= set(no_id(plain)) and 0 < len(got) <= len(plain)
    assert all(l.split(",")[3] in case["targets"][::2] for l in got)
