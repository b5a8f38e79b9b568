"""`ris` with the pages of a batch shared out over the workers (PRB_SPLIT): the output of every mode is byte for byte
what one worker writes, the knob is checked before any GPU work, and the split reports itself only when asked for.

Shapes: three pages of 300 random 300-nt targets (`db -c`), three queries of 600-900 nt - one batch - the last of them
poly-A, which has no hit under -g -9; two workers on device 0."""
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# mode -> (the switches, whether the file is binary and compared after `txt`)
MODES = {
    "s0": (["-s", "0"], False),
    "s1": (["-s", "1"], False),
    "b_txt": (["-b"], True),
    "t": (["-t"], False),
    "t_n2": (["-t", "-n", "2"], False),
    "q": (["-q"], False),
    "k3": (["-k", "3"], False),
    "k3_b_txt": (["-k", "3", "-b", "-s", "1"], True),
}
SPLIT_LINE = re.compile(r"^page split: (\d+) batch\(es\), pages per worker: ([0-9,]+)$", re.M)


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_unknown_split_value_is_refused_before_any_gpu_work(tmp_path):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"), "-d",
                        str(tmp_path / "nodb")], capture_output=True, text=True, env=clean_env(PRB_SPLIT="bogus"))
    assert r.returncode == 1
    assert (r.stderr.splitlines() or [""])[0] == 'Error: PRB_SPLIT needs one of auto, queries or pages (got "bogus")'
    assert not (tmp_path / "out").exists()


def test_usage_names_the_knob():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "PRB_SPLIT=auto|queries|pages" in text and "ignored with WORLD_SIZE > 1" in text


def random_seq(rng, n):
    return "".join(np.array(list("ACGU"))[rng.integers(0, 4, n)])


class Bench:
    def __init__(self, tmp):
        from priblast_amd import capi
        self.capi, self.tmp = capi, tmp
        rng = np.random.default_rng(21)
        targets = [random_seq(rng, 300) for _ in range(900)]
        queries = [random_seq(rng, 900), random_seq(rng, 600), "A" * 700]
        self.fa = str(tmp / "q.fa")
        with open(self.fa, "w") as f:
            for i, q in enumerate(queries):
                f.write(f">query{i}\n{q}\n")
        dbfa = str(tmp / "db.fa")
        with open(dbfa, "w") as f:
            for i, t in enumerate(targets):
                f.write(f">target{i}\n{t}\n")
        self.db3, self.db1 = str(tmp / "db3"), str(tmp / "db1")
        for prefix, chunk in ((self.db3, ["-c", "300"]), (self.db1, [])):
            subprocess.run([capi.BIN_PATH, "db", "-i", dbfa, "-o", prefix] + chunk, check=True, env=clean_env())
        self.count = 0
        self.base = {}

    def ris(self, mode, db=None, **env):
        """-> (the text of the output, after `txt` for the binary modes; stderr)"""
        switches, binary = MODES[mode]
        self.count += 1
        out = str(self.tmp / f"out{self.count}")
        r = subprocess.run([self.capi.BIN_PATH, "ris", "-i", self.fa, "-o", out, "-d", db or self.db3, "-g", "-9"] + switches,
                           capture_output=True, text=True, env=clean_env(**env))
        assert r.returncode == 0, r.stderr
        if binary:
            subprocess.run([self.capi.BIN_PATH, "txt", "-i", out, "-o", out + ".txt"], check=True)
            with open(out, "rb") as f:
                raw = f.read()
            out += ".txt"
        with open(out, "rb") as f:
            text = f.read()
        return (text, raw) if binary else (text,), r.stderr

    def baseline(self, mode):
        if mode not in self.base:
            self.base[mode] = self.ris(mode, PRB_DEVICES="0")
        return self.base[mode]


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    return Bench(tmp_path_factory.mktemp("split"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_split_output_is_byte_identical(bench, mode):
    want, err = bench.baseline(mode)
    assert want[0].count(b"\n") > 3 and b"query2" not in want[0]  # (lines beyond the header; none of the poly-A query)
    assert "page split" not in err
    got, err = bench.ris(mode, PRB_DEVICES="0,0", PRB_SPLIT="pages")
    assert got == want
    m = SPLIT_LINE.search(err)
    assert m and m.group(1) == "1", err
    per = [int(x) for x in m.group(2).split(",")]
    assert len(per) == 2 and sum(per) == 3 and min(per) >= 1, err  # (worker k begins with page k)
    got, err = bench.ris(mode, PRB_DEVICES="0,0")  # auto: one batch for two workers
    assert got == want
    assert "page split" not in err


@pytest.mark.gpu
def test_split_of_every_batch_and_the_other_settings(bench):
    mode = "t_n2"
    want, _ = bench.baseline(mode)
    # three batches of one query, each split over three workers
    got, err = bench.ris(mode, PRB_DEVICES="0,0,0", PRB_SPLIT="pages", PRB_BATCH="1")
    assert got == want
    m = SPLIT_LINE.search(err)
    assert m and m.group(1) == "3" and sum(int(x) for x in m.group(2).split(",")) == 9, err
    # queries: today's path, nothing reported
    got, err = bench.ris(mode, PRB_DEVICES="0,0", PRB_SPLIT="queries")
    assert got == want and "page split" not in err
    # a database of one page: `pages` falls back silently
    one, err1 = bench.ris(mode, db=bench.db1, PRB_DEVICES="0")
    got, err = bench.ris(mode, db=bench.db1, PRB_DEVICES="0,0", PRB_SPLIT="pages")
    assert got == one and "page split" not in err and err == err1
