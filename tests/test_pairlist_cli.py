"""`ris -L FILE`: the refusals of a faulty pair list - before any GPU work, so they run without one - and, on the GPU,
the runs: a -L run writes the lines of the plain run for the listed pairs, whatever else the command line asks for.

Lines are compared without their Id.  The base pairs of a query's first line keep the order they were found in (SURVEY
a17), and the first line of a query under -L is another one than in the full run: for a line that is the first of its
query in either run the base pairs are compared as sorted lists, for every other line as text."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, out="out", queries=QUERIES, **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", queries, "-o", str(tmp_path / out), "-d", db] + extra, capture_output=True,
                          text=True, env=clean_env(**env))


# ------------------------------------------------------------------------- refusals (no GPU)
REFUSALS = {
    "no_tab": ("mq0 mdb1\n", "Error: pair list line 1: expected query name, one tab, target name"),
    "two_tabs": ("# a comment\n\nmq0\tmdb1\nmq0\tmdb1\textra\n", "Error: pair list line 4: expected query name, one tab, target name"),
    "unknown_query": ("mq0\tmdb1\r\nmq9\tmdb1\r\n", 'Error: pair list line 2: no query is named "mq9"'),
    "unknown_target": ("*\tmdb1\nmq1\tmdb99\n", 'Error: pair list line 2: no database sequence is named "mdb99"'),
    "star_is_no_target": ("mq1\t*\n", 'Error: pair list line 1: no database sequence is named "*"'),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_a_faulty_list_is_refused_before_any_gpu_work(tmp_path, golden_dir, case):
    text, want = REFUSALS[case]
    (tmp_path / "pairs.tsv").write_bytes(text.encode())
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-L", str(tmp_path / "pairs.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_an_unreadable_or_empty_list_is_refused(tmp_path, golden_dir):
    db = os.path.join(golden_dir, "mixdb")
    r = ris(tmp_path, db, ["-L", str(tmp_path / "missing.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == "Error: can't open the pair list (-L): " + str(tmp_path / "missing.tsv")
    assert r.returncode == 1 and not (tmp_path / "out").exists()
    (tmp_path / "none.tsv").write_text("# nothing but a comment\n\n\r\n")
    r = ris(tmp_path, db, ["-L", str(tmp_path / "none.tsv")])
    assert (r.stderr.splitlines() or [""])[0] == "Error: the pair list (-L) allows no pair: " + str(tmp_path / "none.tsv")
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_usage_names_the_switch():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-L STR" in text and "query name, a tab" in text


# ------------------------------------------------------------------------- runs (GPU)
LIST = ("# the listed pairs\r\n"
        "mq0\tmdb14\r\n"
        "\r\n"
        "mq1\tmdb3\n"
        "mq1\tmdb3\n"       # a pair twice
        "mq1\tmdb14\n"
        "*\tmdb7\n"         # every query
        "mq_rc\tmdb0\n"
        "mq3\tmdb20\n")


def listed(qname, tname):
    pairs = {("mq0", "mdb14"), ("mq1", "mdb3"), ("mq1", "mdb14"), ("mq_rc", "mdb0"), ("mq3", "mdb20")}
    return tname == "mdb7" or (qname, tname) in pairs


def records(path):
    """the result lines as (query name, target name, the fields between, base pairs) with a first-of-query flag"""
    with open(path) as f:
        lines = f.read().splitlines()[3:]
    out, seen_q = [], None
    for k, l in enumerate(lines):
        f = l.split(",")
        assert f[0] == str(k), (k, l)  # Id counts the written lines
        out.append(dict(q=f[1], t=f[3], mid=f[2:8], bp=f[8].split(), first=f[1] != seen_q))
        seen_q = f[1]
    return out


def assert_listed_lines(got_path, plain_path, what):
    got = records(got_path)
    want = [r for r in records(plain_path) if listed(r["q"], r["t"])]
    assert len(got) == len(want) > 0, (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["q"], g["t"], g["mid"]) == (w["q"], w["t"], w["mid"]), (what, k)
        if g["first"] or w["first"]:
            assert sorted(g["bp"]) == sorted(w["bp"]), (what, k)
        else:
            assert g["bp"] == w["bp"], (what, k)
    return len(got)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden_dir):
    """queries: mix's, with mq1 once more under the same name; the plain run's lines, once"""
    tmp = tmp_path_factory.mktemp("pairlist_cli")
    with open(QUERIES) as f:
        text = f.read()
    at = text.index(">mq1\n")
    (tmp / "q.fa").write_text(text + text[at:text.index(">mq2\n")])
    (tmp / "pairs.tsv").write_bytes(LIST.encode())
    db = os.path.join(golden_dir, "mixdb")
    for s in ("0", "1"):
        r = ris(tmp, db, ["-s", s], out=f"plain{s}", queries=str(tmp / "q.fa"))
        assert r.returncode == 0, r.stderr
    return dict(tmp=tmp, db=db, q=str(tmp / "q.fa"), list=str(tmp / "pairs.tsv"))


@pytest.mark.gpu
@pytest.mark.parametrize("style", ["0", "1"])
def test_listed_pairs_get_the_plain_runs_lines(runs, style):
    tmp = runs["tmp"]
    r = ris(tmp, runs["db"], ["-s", style, "-L", runs["list"]], out=f"listed{style}", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    n = assert_listed_lines(tmp / f"listed{style}", tmp / f"plain{style}", style)
    with open(tmp / f"plain{style}") as f, open(tmp / f"listed{style}") as g:
        a, b = f.read().splitlines(), g.read().splitlines()
    assert a[:3] == b[:3]  # the header is unchanged
    names = [r["q"] for r in records(tmp / f"listed{style}")]
    assert names.count("mq1") > 0 and n < len(a) - 3
    print("lines", n, "of", len(a) - 3)


@pytest.mark.gpu
@pytest.mark.parametrize("style", ["0", "1"])
def test_a_list_of_every_pair_writes_the_plain_runs_bytes(runs, style):
    """every target for every query: the file of the run without -L, byte for byte"""
    tmp = runs["tmp"]
    with open(os.path.join(GOLDEN, "mix_db.fa")) as f:
        targets = [l[1:].strip() for l in f if l.startswith(">")]
    (tmp / "all.tsv").write_text("".join(f"*\t{t}\n" for t in targets))
    r = ris(tmp, runs["db"], ["-s", style, "-L", str(tmp / "all.tsv")], out=f"all{style}", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    a = (tmp / f"all{style}").read_bytes()
    assert a == (tmp / f"plain{style}").read_bytes() and a.count(b"\n") > 10


@pytest.mark.gpu
def test_binary_then_txt_gives_the_same_text(runs):
    from priblast_amd import capi
    tmp = runs["tmp"]
    r = ris(tmp, runs["db"], ["-s", "1", "-L", runs["list"]], out="text1", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    r = ris(tmp, runs["db"], ["-s", "1", "-b", "-L", runs["list"]], out="bin1", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    subprocess.run([capi.BIN_PATH, "txt", "-i", str(tmp / "bin1"), "-o", str(tmp / "bin1.txt")], check=True, env=clean_env())
    assert (tmp / "bin1.txt").read_bytes() == (tmp / "text1").read_bytes()


@pytest.mark.gpu
def test_small_batches_and_summary_lines(runs):
    """batches of two queries - a mask per batch, one of them with the `*` line alone - and -t over the restricted list"""
    tmp = runs["tmp"]
    r = ris(tmp, runs["db"], ["-s", "1", "-L", runs["list"]], out="b2", queries=runs["q"], PRB_BATCH="2")
    assert r.returncode == 0, r.stderr
    assert_listed_lines(tmp / "b2", tmp / "plain1", "PRB_BATCH=2")
    r = ris(tmp, runs["db"], ["-t"], out="t_plain", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    r = ris(tmp, runs["db"], ["-t", "-L", runs["list"]], out="t_listed", queries=runs["q"])
    assert r.returncode == 0, r.stderr
    # (without Id and without the best hit's end pairs: they are the ends of its list, which for a query's first hit is in
    #  found order - see the head of this file)
    strip = lambda p: [l.split(",", 1)[1].rsplit(",", 1)[0] for l in open(p).read().splitlines()[3:]]
    want = [l for l in strip(tmp / "t_plain") if listed(l.split(",")[0], l.split(",")[2])]
    assert strip(tmp / "t_listed") == want and len(want) > 3


@pytest.mark.gpu
def test_two_workers_sharing_pages_write_the_same_bytes(runs, tmp_path):
    """a database of several pages (`db -c`); PRB_DEVICES=0,0 PRB_SPLIT=pages: each worker builds the mask of its batch"""
    from priblast_amd import capi
    db = str(tmp_path / "db3")
    subprocess.run([capi.BIN_PATH, "db", "-i", os.path.join(GOLDEN, "mix_db.fa"), "-o", db, "-c", "10"], check=True, env=clean_env())
    one = ris(tmp_path, db, ["-s", "1", "-L", runs["list"]], out="one", queries=runs["q"])
    two = ris(tmp_path, db, ["-s", "1", "-L", runs["list"]], out="two", queries=runs["q"], PRB_DEVICES="0,0", PRB_SPLIT="pages")
    assert one.returncode == 0 and two.returncode == 0, (one.stderr, two.stderr)
    assert "page split:" in two.stderr
    a = (tmp_path / "one").read_bytes()
    assert a == (tmp_path / "two").read_bytes() and a.count(b"\n") > 6
    plain = ris(tmp_path, db, ["-s", "1"], out="plain", queries=runs["q"])
    assert plain.returncode == 0, plain.stderr
    assert_listed_lines(tmp_path / "one", tmp_path / "plain", "pages")


@pytest.mark.gpu
def test_two_ranks_write_the_same_lines(runs, tmp_path):
    from test_gpu_multirank import FAKE, _env, _wait_all
    from priblast_amd import capi
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "fake_rccl")], check=True)
    common = ["-i", runs["q"], "-d", runs["db"], "-s", "1", "-L", runs["list"]]
    one = str(tmp_path / "one.txt")
    subprocess.run([capi.BIN_PATH, "ris", "-o", one] + common, check=True, env=_env(tmp_path, FAKE, PRB_BATCH="2"))
    (tmp_path / "rdv").mkdir()
    out = str(tmp_path / "ranked.txt")
    procs = []
    for r in range(2):
        env = _env(tmp_path, FAKE, PRB_BATCH="2", WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0", PRB_DEVICES="0", MASTER_PORT="29741")
        procs.append(subprocess.Popen([capi.BIN_PATH, "ris", "-o", out, "-p", str(tmp_path / "rdv")] + common, env=env))
    assert _wait_all(procs, 300) == [0, 0]
    with open(one, "rb") as f, open(out, "rb") as g:
        a, b = f.read(), g.read()
    assert a.count(b"\n") > 6 and a == b
