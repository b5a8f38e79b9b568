"""`ris -j` on the planted case of test_gpu_chain.py: its lines are the plain run's lines that the rule keeps, and it
combines with -t, -t -n, -q, -k, -r, -c, -b and PRB_SPLIT.  The yardstick is the plain hit path filtered in Python
(chain_ref)."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_coverage as cov
import test_gpu_targets as tgt
from chain_ref import filter_page
from distinct_ref import planted_sequences
from test_gpu_distinct import RELAXED, pair_records, search
from test_gpu_profile import profile
from test_gpu_top import rank
from test_gpu_tophits import Ranking, open_batch

FLAGS = ["-f", "-3", "-g", "-6.5"]  # test_gpu_distinct.RELAXED
REGION_COLUMNS = "Id,Target name,Target Length,Start,End,Hits,Max Hits,Max Queries,Peak,Minimum Interaction Energy,Query name,Query Length,BasePair"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the planted case, its plain hits, what the rule keeps of them, and the text of every table mode over the kept
    hits - the bodies only, written by the library's formatters from records reduced in Python"""
    from priblast_amd import capi
    d = tmp_path_factory.mktemp("chain_cli")
    qnames, queries, tnames, targets = planted_sequences()
    assert len(queries[0]) > len(queries[1])  # (the command line takes the longest query first: the same order)
    prefix, fasta = str(d / "pdb"), str(d / "q.fa")
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in zip(qnames, queries)))
    with capi.Context(0) as ctx:
        capi.db_build(ctx, prefix, tnames, targets, page_size=7)
        db, qb = open_batch(ctx, prefix, queries)
        try:
            plain = {s: search(ctx, qb, db, capi.default_opts(output_style=s, **RELAXED)) for s in (0, 1)}
            kept = {s: [filter_page(h, bp) for h, bp, _ in plain[s]] for s in (0, 1)}
            qlen = [qb.length_unmasked(q) for q in range(len(queries))]
            ids = np.arange(len(queries), dtype=np.int32)
            pair_pages = [pair_records(h, bp) for h, bp, _ in kept[0]]
            info = cov.seq_info(db)
            records = {
                "t": (capi.write_summary_lines, pair_pages),
                "tn3": (capi.write_top_lines, rank(pair_pages, 3)),
                "q": (capi.write_profile_lines, profile([(p, h, bp[h["bp_offset"]], bp[h["bp_offset"] + 1]) for p, (h, bp, _) in enumerate(kept[0])],
                                                        [len(q) for q in queries])),
                "r3": (capi.write_target_lines, tgt.rank([(ids, p, recs) for p, recs in enumerate(pair_pages)], 3)),
                "c1": (capi.write_region_lines, cov.regions(cov.table([(ids, p, h, bp) for p, (h, bp, _) in enumerate(kept[0])], info), info, 1)),
            }
            text = {}
            for name, (write, recs) in records.items():
                path = str(d / f"want_{name}.txt")
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
                try:
                    lines, _ = write(db, qnames, qlen, recs, 0, fd)
                    assert lines > 0
                finally:
                    os.close(fd)
                with open(path) as f:
                    text[name] = f.read()
            names = {(p, i): db.seq_name(p, i) for p in range(db.npages) for i in range(db.page_info(p)[0])}
        finally:
            qb.close()
            db.close()
    return dict(dir=d, prefix=prefix, fasta=fasta, qnames=qnames, plain=plain, kept=kept, text=text, names=names)


def ris(case, name, extra, env_extra=None):
    from priblast_amd import capi
    out = str(case["dir"] / name)
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        if k not in (env_extra or {}):
            env.pop(k, None)
    subprocess.run([capi.BIN_PATH, "ris", "-i", case["fasta"], "-o", out, "-d", case["prefix"]] + FLAGS + list(extra), check=True,
                   env=env, timeout=600)
    return out


def read(path):
    with open(path) as f:
        return f.read()


def body(text):
    """-> (the three header lines, the lines without their Id) - the Ids must count from 0"""
    lines = text.splitlines()
    assert [int(l.split(",", 1)[0]) for l in lines[3:]] == list(range(len(lines) - 3))
    return lines[:3], [l.split(",", 1)[1] for l in lines[3:]]


def test_usage_names_the_chain_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -j " in r.stdout and "co-linear" in r.stdout


def refused(tmp_path, switches):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", str(tmp_path / "q.fa"), "-o", str(tmp_path / "out"), "-d", str(tmp_path / "nodb")] + switches,
                       capture_output=True, text=True)
    assert r.returncode != 0 and not (tmp_path / "out").exists()
    return r.stderr


def test_j_is_refused_with_u_before_any_gpu_work(tmp_path):
    """neither the input nor the database exists: the refusal comes from the command line alone"""
    for switches in (["-u", "-j"], ["-j", "-u"], ["-j", "-u", "-t"]):
        err = refused(tmp_path, switches)
        assert "-j (the best co-linear chain of sites of each pair)" in err and "-u (the distinct interaction sites of each pair)" in err
        assert "can't be combined" in err


def test_j_is_still_refused_where_its_partner_is(tmp_path):
    """-j adds no other refusal and lifts none: -t -b, -q -t and -n alone stay refused with it, and nothing is written"""
    err = refused(tmp_path, ["-j", "-t", "-b"])
    assert "-t" in err and "-b" in err and "-j" not in err
    err = refused(tmp_path, ["-j", "-q", "-t"])
    assert "-q" in err and "-t" in err and "-j" not in err
    err = refused(tmp_path, ["-j", "-n", "3"])
    assert "-n" in err and "needs" in err


@pytest.mark.gpu
@pytest.mark.parametrize("style", [0, 1])
def test_j_keeps_the_plain_lines_of_the_kept_hits(case, style):
    head, plain = body(read(ris(case, f"plain{style}.txt", ["-s", str(style)])))
    flags = []  # the keep flags in line order: query by query, page by page, the page's hits in order
    for q in range(len(case["qnames"])):
        for (h, _, _), (_, _, keep) in zip(case["plain"][style], case["kept"][style]):
            flags += keep[h["query"] == q].tolist()
    assert len(flags) == len(plain) and not all(flags)
    text = read(ris(case, f"j{style}.txt", ["-j", "-s", str(style)]))
    jhead, jlines = body(text)
    assert jhead == head
    assert jlines == [l for l, k in zip(plain, flags) if k]
    if style == 1:  # -b -j writes ordinary records: `txt` gives the text of -j
        from priblast_amd import capi
        back = str(case["dir"] / "back.txt")
        subprocess.run([capi.BIN_PATH, "txt", "-i", ris(case, "j.prb", ["-j", "-s", "1", "-b"]), "-o", back], check=True, timeout=600)
        assert read(back) == text


def lines_behind_the_header(text):
    return "\n".join(text.splitlines()[3:]) + "\n"


@pytest.mark.gpu
@pytest.mark.parametrize("name,switches", [("t", ["-t"]), ("tn3", ["-t", "-n", "3"]), ("q", ["-q"]), ("r3", ["-r", "3"]), ("c1", ["-c", "1"])])
def test_j_with_the_table_modes(case, name, switches):
    got = read(ris(case, f"{name}_j.txt", switches + ["-j"]))
    assert lines_behind_the_header(got) == case["text"][name]
    if name == "c1":
        assert got.splitlines()[2] == REGION_COLUMNS


@pytest.mark.gpu
def test_j_with_the_best_hits(case):
    """-k 5 -j -s 1: the five best kept hits per query, lines of the plain -s 1 run"""
    _, plain = body(read(ris(case, "plain_s1.txt", ["-s", "1"])))
    _, lines = body(read(ris(case, "k5j.txt", ["-k", "5", "-j", "-s", "1"])))
    assert set(lines) <= set(plain)
    want = [(case["qnames"][int(r["query"])], case["names"][(int(r["page"]), int(r["db_id"]))], "%g" % r["e_tot"])
            for r in Ranking([(h, bp) for h, bp, _ in case["kept"][1]]).cut(5)[0]]
    assert [(l.split(",")[0], l.split(",")[2], l.split(",")[6]) for l in lines] == want


@pytest.mark.gpu
def test_j_with_the_pages_split_over_two_workers(case):
    split = {"PRB_DEVICES": "0,0", "PRB_SPLIT": "pages"}
    for name, extra in (("j", ["-j"]), ("k5j", ["-k", "5", "-j"])):
        one = read(ris(case, f"one_{name}.txt", extra))
        assert len(one.splitlines()) > 3
        assert read(ris(case, f"two_{name}.txt", extra, split)) == one
