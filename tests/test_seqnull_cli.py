"""`ris -t -z N -H H -D R [-Z SEED]` on the GPU: the lines against tests/seqnull_ref.py - whose summaries come from
capi.search_page_summary and whose lines from null_ref.lines, not from the new code -, the same bytes however the run is
cut or masked, the bytes of plain `-z N` when no pair can retire, and every line found verbatim in the output of the
merged `ris -t -z Seen`.  A batch holds its queries longest first, a decoy is shuffled with its query's place in the
input file, and the lines of a batch come by query (in batch order), then page, then target.  (The refusals and the usage
text need no GPU: tests/test_seqnull_host.py.)"""
import os
import subprocess

import pytest

import null_ref
import refdump
import seqnull_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")
N, H, R, SEED = 6, 1, 2, 1
ARGS = ["-t", "-z", str(N), "-H", str(H), "-D", str(R), "-Z", str(SEED)]
LISTED = [("mq0", "mdb14"), ("mq1", "mdb3"), ("mq1", "mdb14"), ("mq_rc", "mdb0"), ("mq3", "mdb20")]  # (test_null_cli.py's list)
EVERY = ["mdb7"]


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, out="out", **env):
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / out), "-d", db] + extra, capture_output=True, text=True,
                       env=clean_env(**env))
    assert r.returncode == 0, r.stderr
    return r


def body(path):
    with open(path) as f:
        text = f.read()
    head = text.split("\n", 3)
    assert head[2].endswith("BasePair, Decoys, Null Hits, Null LE, Null Minimum Energy, P Value")
    return head[3]


def seen_of(line):
    return int(line.rsplit(",", 5)[1])


class Mix:
    """the golden mix database and queries as a run batches them, open for the reference's searches"""

    def __init__(self, golden_dir):
        from priblast_amd import capi
        names, seqs = refdump.read_fasta(QUERIES)
        self.order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))  # (stable: equal lengths keep their file order)
        self.bn, self.bs = [names[i] for i in self.order], [seqs[i] for i in self.order]
        self.ctx = capi.Context(0)
        self.db = capi.Db(self.ctx, os.path.join(golden_dir, "mixdb"))
        self.qb = capi.QBatch(self.ctx, self.bs, self.db.repeat_flag)
        self.qb.accessibility(self.db.W, self.db.delta)
        self.qlens = [self.qb.length_unmasked(q) for q in range(len(self.bs))]

    def summaries(self, opts=None):
        return seqnull_ref.summaries(self.ctx, self.qb, self.bs, self.db, N, seed=SEED, file_pos=self.order, opts=opts)

    def lines(self, recs):
        return null_ref.lines(self.db, self.bn, self.qlens, recs)

    def close(self):
        self.qb.close()
        self.db.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def want_u(golden_dir):
    """the reference's lines for mix with -u"""
    from priblast_amd import capi
    m = Mix(golden_dir)
    try:
        return m.lines(seqnull_ref.fold(*m.summaries(capi.default_opts(distinct_sites=1)), N, H, R))
    finally:
        m.close()


@pytest.fixture(scope="module")
def want(golden_dir):
    """the reference's lines for mix: the whole run, the run of plain -z N and the run under the pair list; and the
    summaries of the whole run"""
    from priblast_amd import capi
    out = {}
    m = Mix(golden_dir)
    try:
        ctx, db, qb, bn, qlens = m.ctx, m.db, m.qb, m.bn, m.qlens
        real, decoys = m.summaries()
        out["lists"] = (real, decoys)
        out["run"] = m.lines(seqnull_ref.fold(real, decoys, N, H, R))
        out["plain"] = m.lines(null_ref.fold(real, decoys, N))
        mq, mp, md = [], [], []
        for p in range(db.npages):
            for i in range(db.page_info(p)[0]):
                for k, qn in enumerate(bn):
                    if db.seq_name(p, i) in EVERY or (qn, db.seq_name(p, i)) in LISTED:
                        mq.append(k), mp.append(p), md.append(i)
        with capi.PairMask(ctx, qb, db) as pm:
            pm.allow(mq, mp, md)
            listed = {p: capi.search_page_summary(ctx, qb, db, p, capi.default_opts(allowed_pairs=pm.h.value)) for p in range(db.npages)}
        out["listed"] = m.lines(seqnull_ref.fold(listed, decoys, N, H, R))  # (the decoys are the run's own)
    finally:
        m.close()
    return out


@pytest.fixture(scope="module")
def run(golden_dir, tmp_path_factory):
    """`ris -t -z N -H H -D R -Z SEED` on mix, once: (the output file's bytes, its lines, stderr)"""
    d = tmp_path_factory.mktemp("seqnull_run")
    r = ris(d, os.path.join(golden_dir, "mixdb"), ARGS)
    return (d / "out").read_bytes(), body(d / "out"), r.stderr


def test_the_reference_shows_every_case(want):
    """on null_ref's own fold of the summaries: a pair retired at the first boundary, one at a later boundary before N,
    one never retired, and a retired pair whose -z N line differs from its -z Seen line"""
    real, decoys = want["lists"]
    assert seqnull_ref.shows_every_case(real, decoys, N, H, R) == {"first": True, "later": True, "never": True, "differs": True}
    run, plain = want["run"].splitlines(), want["plain"].splitlines()
    assert len(run) == len(plain) > 10 and {seen_of(l) for l in run} == set(seqnull_ref.boundaries(N, R))
    assert any(seen_of(a) < N and a.rsplit(",", 5)[2:] != b.rsplit(",", 5)[2:] for a, b in zip(run, plain))


def test_lines_equal_the_reference(run, want):
    assert run[1] == want["run"]
    assert "live pairs after decoy 2: " in run[2] and ", 4: " in run[2] and ", 6: " in run[2]


@pytest.mark.parametrize("env", [dict(PRB_BATCH="1"), dict(PRB_NULL_MASK="0"), dict(PRB_SPLIT="pages")], ids=lambda e: "_".join(e))
def test_same_bytes_however_the_run_is_cut_or_masked(tmp_path, golden_dir, run, env):
    ris(tmp_path, os.path.join(golden_dir, "mixdb"), ARGS, **env)
    assert (tmp_path / "out").read_bytes() == run[0]


def test_with_distinct_sites(tmp_path, golden_dir, want_u):
    ris(tmp_path, os.path.join(golden_dir, "mixdb"), ARGS + ["-u"])
    assert body(tmp_path / "out") == want_u and want_u.count("\n") > 10


def test_under_a_pair_list(tmp_path, golden_dir, want):
    db = os.path.join(golden_dir, "mixdb")
    (tmp_path / "pairs.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in LISTED) + "".join(f"*\t{t}\n" for t in EVERY))
    ris(tmp_path, db, ARGS + ["-L", str(tmp_path / "pairs.tsv")])
    assert body(tmp_path / "out") == want["listed"] and 0 < want["listed"].count("\n") < want["run"].count("\n")
    ris(tmp_path, db, ARGS + ["-L", str(tmp_path / "pairs.tsv")], out="nomask", PRB_NULL_MASK="0")
    assert (tmp_path / "nomask").read_bytes() == (tmp_path / "out").read_bytes()


def test_without_retiring_the_bytes_are_those_of_plain_z(tmp_path, golden_dir, want):
    db = os.path.join(golden_dir, "mixdb")
    ris(tmp_path, db, ["-t", "-z", str(N), "-Z", str(SEED)], out="z")
    ris(tmp_path, db, ["-t", "-z", str(N), "-Z", str(SEED), "-H", str(N), "-D", str(N)], out="h")
    assert (tmp_path / "h").read_bytes() == (tmp_path / "z").read_bytes() and body(tmp_path / "z") == want["plain"]


@pytest.mark.parametrize("b", seqnull_ref.boundaries(N, R))
def test_every_line_is_a_line_of_z_seen(tmp_path, golden_dir, run, b):
    """ties the feature to the merged -z: the lines of the pairs with Seen = b are lines of `ris -t -z b`"""
    ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-z", str(b), "-Z", str(SEED)])
    theirs = set(body(tmp_path / "out").splitlines())
    at_b = [l for l in run[1].splitlines() if seen_of(l) == b]
    assert at_b and all(l in theirs for l in at_b)
