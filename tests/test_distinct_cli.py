"""`ris -u` on the planted case of test_gpu_distinct.py: its lines are the plain run's lines that the rule keeps, and it
combines with -k, -t, -q, -b and PRB_SPLIT.  The yardstick is the plain hit path filtered in Python (distinct_ref)."""
import os
import subprocess

import numpy as np
import pytest

from distinct_ref import filter_page, planted_sequences
from test_gpu_distinct import RELAXED, pair_records, search
from test_gpu_profile import profile
from test_gpu_tophits import Ranking, open_batch

FLAGS = ["-f", "-3", "-g", "-6.5"]  # test_gpu_distinct.RELAXED


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from priblast_amd import capi
    d = tmp_path_factory.mktemp("distinct_cli")
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
            text = {}
            for name, rows in (("t", None), ("q", profile([(p, h, bp[h["bp_offset"]], bp[h["bp_offset"] + 1])
                                                           for p, (h, bp, _) in enumerate(kept[0])], [len(q) for q in queries]))):
                path = str(d / f"want_{name}.txt")
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
                try:
                    if name == "t":
                        capi.write_summary_lines(db, qnames, qlen, [pair_records(h, bp) for h, bp, _ in kept[0]], 0, fd)
                    else:
                        capi.write_profile_lines(db, qnames, qlen, rows, 0, fd)
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


def test_usage_names_the_distinct_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -u " in r.stdout


def test_u_is_still_refused_where_its_partner_is(tmp_path):
    """-u adds no refusal and lifts none: -t -b stays refused with it, and nothing is written"""
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", str(tmp_path / "q.fa"), "-o", str(tmp_path / "out"), "-d", str(tmp_path / "nodb"),
                        "-u", "-t", "-b"], capture_output=True, text=True)
    assert r.returncode != 0 and "-t" in r.stderr and "-b" in r.stderr and not (tmp_path / "out").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("style", [0, 1])
def test_u_keeps_the_plain_lines_of_the_kept_hits(case, style):
    head, plain = body(read(ris(case, f"plain{style}.txt", ["-s", str(style)])))
    flags = []  # the keep flags in line order: query by query, page by page, the page's hits in order
    for q in range(len(case["qnames"])):
        for (h, _, _), (_, _, keep) in zip(case["plain"][style], case["kept"][style]):
            flags += keep[h["query"] == q].tolist()
    assert len(flags) == len(plain) and not all(flags)
    text = read(ris(case, f"u{style}.txt", ["-u", "-s", str(style)]))
    uhead, ulines = body(text)
    assert uhead == head
    assert ulines == [l for l, k in zip(plain, flags) if k]
    if style == 1:  # -b -u writes ordinary records: `txt` gives the text of -u
        from priblast_amd import capi
        back = str(case["dir"] / "back.txt")
        subprocess.run([capi.BIN_PATH, "txt", "-i", ris(case, "u.prb", ["-u", "-s", "1", "-b"]), "-o", back], check=True, timeout=600)
        assert read(back) == text


@pytest.mark.gpu
def test_u_with_the_table_modes(case):
    assert "\n".join(read(ris(case, "tu.txt", ["-t", "-u"])).splitlines()[3:]) + "\n" == case["text"]["t"]
    assert "\n".join(read(ris(case, "qu.txt", ["-q", "-u"])).splitlines()[3:]) + "\n" == case["text"]["q"]
    # -k 5 -u -s 1: the five best kept hits per query, lines of the plain -s 1 run
    _, plain = body(read(ris(case, "plain_s1.txt", ["-s", "1"])))
    _, lines = body(read(ris(case, "k5u.txt", ["-k", "5", "-u", "-s", "1"])))
    assert set(lines) <= set(plain)
    want = [(case["qnames"][int(r["query"])], case["names"][(int(r["page"]), int(r["db_id"]))], "%g" % r["e_tot"])
            for r in Ranking([(h, bp) for h, bp, _ in case["kept"][1]]).cut(5)[0]]
    assert [(l.split(",")[0], l.split(",")[2], l.split(",")[6]) for l in lines] == want


@pytest.mark.gpu
def test_u_with_the_pages_split_over_two_workers(case):
    split = {"PRB_DEVICES": "0,0", "PRB_SPLIT": "pages"}
    for name, extra in (("u", ["-u"]), ("k5u", ["-k", "5", "-u"])):
        one = read(ris(case, f"one_{name}.txt", extra))
        assert len(one.splitlines()) > 3
        assert read(ris(case, f"two_{name}.txt", extra, split)) == one
