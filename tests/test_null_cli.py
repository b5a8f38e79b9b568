"""`ris -t -z N [-Z SEED]`: the refusals - before any GPU work, so they run without one - and, on the GPU, the runs
against the lines of tests/null_ref.py.  A batch holds its queries longest first, a decoy is shuffled with its query's
place in the input file, and the lines of a batch come by query (in batch order), then page, then target."""
import os
import subprocess

import numpy as np
import pytest

import null_ref
import refdump

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
QUERIES = os.path.join(GOLDEN, "mix_q.fa")

Z = "-z (an empirical p-value per pair from N shuffled decoys)"
REFUSALS = {
    "-z 3": f"Error: {Z} needs -t (per-pair summary lines)",
    "-t -z 3 -n 2": f"Error: {Z} can't be combined with -n (the N best pairs per query)",
    "-t -z 3 -k 2": f"Error: {Z} can't be combined with -k (the N best interaction sites per query)",
    "-z 3 -q": f"Error: {Z} can't be combined with -q (per-position profile lines)",
    "-z 3 -r 2": f"Error: {Z} can't be combined with -r (the N best queries per target)",
    "-z 3 -c 2": f"Error: {Z} can't be combined with -c (the regions of each target bound by at least D queries)",
    "-t -z 3 -b": f"Error: {Z} can't be combined with -b (binary hit records)",
    "-t -Z 5": f"Error: -Z (the seed of the decoys' shuffles) needs {Z}",
    "-Z 5": f"Error: -Z (the seed of the decoys' shuffles) needs {Z}",
    "-t -z 0": "Error: -z needs an integer between 1 and 100000 (this build's limit)",
    "-t -z 100001": "Error: -z needs an integer between 1 and 100000 (this build's limit)",
    "-t -z many": "Error: -z needs an integer between 1 and 100000 (this build's limit)",
    "-t -z 3 -Z -1": "Error: -Z needs a non-negative integer",
    "-t -z 3 -Z x": "Error: -Z needs a non-negative integer",
}


def clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM", "PRB_SPLIT", "PRB_DEVICES", "PRB_BATCH", "PRB_NULL_MASK"):
        env.pop(k, None)
    env.update(kw)
    return env


def ris(tmp_path, db, extra, out="out", **env):
    from priblast_amd import capi
    return subprocess.run([capi.BIN_PATH, "ris", "-i", QUERIES, "-o", str(tmp_path / out), "-d", db] + extra, capture_output=True,
                          text=True, env=clean_env(**env))


# ------------------------------------------------------------------------- refusals (no GPU)
@pytest.mark.parametrize("extra", list(REFUSALS))
def test_refused_before_any_gpu_work(tmp_path, extra):
    r = ris(tmp_path, str(tmp_path / "nodb"), extra.split())
    assert (r.stderr.splitlines() or [""])[0] == REFUSALS[extra]
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_refused_with_one_process_per_gpu(tmp_path):
    r = ris(tmp_path, str(tmp_path / "nodb"), ["-t", "-z", "3"], WORLD_SIZE="2", RANK="0")
    assert (r.stderr.splitlines() or [""])[0] == f"Error: {Z} is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
    assert r.returncode == 1


def test_usage_names_the_switches():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "-z INT" in text and "-Z INT" in text and "PRB_NULL_MASK" in text


# ------------------------------------------------------------------------- runs (GPU)
LISTED = [("mq0", "mdb14"), ("mq1", "mdb3"), ("mq1", "mdb14"), ("mq_rc", "mdb0"), ("mq3", "mdb20")]
EVERY = ["mdb7"]


def body(path):
    with open(path) as f:
        text = f.read()
    head = text.split("\n", 3)
    assert head[2].endswith("BasePair, Decoys, Null Hits, Null LE, Null Minimum Energy, P Value")
    return head[3]


@pytest.fixture(scope="module")
def want(golden_dir):
    """the lines of null_ref for mix, N = 3, seed 7: the whole run and the run under the pair list"""
    from priblast_amd import capi
    names, seqs = refdump.read_fasta(QUERIES)
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))  # (stable: equal lengths keep their file order)
    bn, bs = [names[i] for i in order], [seqs[i] for i in order]
    out = {}
    with capi.Context(0) as ctx:
        db = capi.Db(ctx, os.path.join(golden_dir, "mixdb"))
        qb = capi.QBatch(ctx, bs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        qlens = [qb.length_unmasked(q) for q in range(len(bs))]
        for seed in (7, 8):
            out[seed] = null_ref.lines(db, bn, qlens, null_ref.null_ref(ctx, qb, bs, db, 3, seed=seed, file_pos=order))
        mq, mp, md = [], [], []
        for p in range(db.npages):
            for i in range(db.page_info(p)[0]):
                for k, qn in enumerate(bn):
                    if db.seq_name(p, i) in EVERY or (qn, db.seq_name(p, i)) in LISTED:
                        mq.append(k), mp.append(p), md.append(i)
        with capi.PairMask(ctx, qb, db) as pm:
            pm.allow(mq, mp, md)
            recs = null_ref.null_ref(ctx, qb, bs, db, 3, seed=7, file_pos=order, real_opts=capi.default_opts(allowed_pairs=pm.h.value))
        out["listed"] = null_ref.lines(db, bn, qlens, recs)
        qb.close()
        db.close()
    return out


@pytest.mark.gpu
def test_lines_equal_the_reference(tmp_path, golden_dir, want):
    db = os.path.join(golden_dir, "mixdb")
    r = ris(tmp_path, db, ["-t", "-z", "3", "-Z", "7"])
    assert r.returncode == 0, r.stderr
    assert body(tmp_path / "out") == want[7] and want[7].count("\n") > 10
    for out, env in (("b1", dict(PRB_BATCH="1")), ("nomask", dict(PRB_NULL_MASK="0", PRB_SPLIT="pages"))):
        r = ris(tmp_path, db, ["-t", "-z", "3", "-Z", "7"], out=out, **env)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / out).read_bytes() == (tmp_path / "out").read_bytes(), env


@pytest.mark.gpu
def test_another_seed_changes_some_count(tmp_path, golden_dir, want):
    r = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-z", "3", "-Z", "8"])
    assert r.returncode == 0, r.stderr
    assert body(tmp_path / "out") == want[8]
    cols = lambda text: [l.rsplit(",", 5)[1:4] for l in text.splitlines()]
    assert len(cols(want[7])) == len(cols(want[8])) and cols(want[7]) != cols(want[8])
    # the seed defaults to 1
    a, b = ris(tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-z", "3"], out="d"), ris(
        tmp_path, os.path.join(golden_dir, "mixdb"), ["-t", "-z", "3", "-Z", "1"], out="d1")
    assert a.returncode == 0 and b.returncode == 0 and (tmp_path / "d").read_bytes() == (tmp_path / "d1").read_bytes()


@pytest.mark.gpu
def test_under_a_pair_list(tmp_path, golden_dir, want):
    db = os.path.join(golden_dir, "mixdb")
    (tmp_path / "pairs.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in LISTED) + "".join(f"*\t{t}\n" for t in EVERY))
    r = ris(tmp_path, db, ["-t", "-z", "3", "-Z", "7", "-L", str(tmp_path / "pairs.tsv")])
    assert r.returncode == 0, r.stderr
    assert body(tmp_path / "out") == want["listed"] and 0 < want["listed"].count("\n") < want[7].count("\n")
    r = ris(tmp_path, db, ["-t", "-z", "3", "-Z", "7", "-L", str(tmp_path / "pairs.tsv")], out="nomask", PRB_NULL_MASK="0")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "nomask").read_bytes() == (tmp_path / "out").read_bytes()
    # the null columns of a listed pair are those of the run without the list
    full = {tuple(l.split(",")[1:5:2]): l.rsplit(",", 5)[1:] for l in want[7].splitlines()}
    for l in want["listed"].splitlines():
        assert full[tuple(l.split(",")[1:5:2])] == l.rsplit(",", 5)[1:], l
