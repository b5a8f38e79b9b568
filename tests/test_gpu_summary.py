"""GPU tests of the per-pair summary mode (prb_search_page_summary, `ris -t`): one record per (query, database
sequence) pair with final hits - hit count, first minimum of the interaction energy with the best hit's energies and
end pairs, left-to-right sum - computed on the device, checked bit for bit against a reduction of the hit path's
records, under the knobs that change how the search is cut up, and on the command line against the reference's
result lines."""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

import refdump
from test_gpu_options import OPTION_SETS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

SUMMARY_COLUMNS = ("Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                   "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair")
OPTS = [{}, OPTION_SETS[1], OPTION_SETS[5]]  # defaults; -f -2 -g -5; -m 2


@pytest.fixture(scope="module")
def ctx():
    from priblast_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def reduce_hits(hits, bp):
    """The contract, restated on the hit path's records (output_style 0): pairs in the order of their first hit."""
    out, where = [], {}
    for i in range(len(hits)):
        h = hits[i]
        key = (int(h["query"]), int(h["db_id"]))
        if key not in where:
            where[key] = len(out)
            out.append(dict(query=key[0], db_id=key[1], hits=0, e_sum=0.0, e_min=None, best=-1, ties=0))
        r = out[where[key]]
        e = float(h["e_tot"])
        r["hits"] += 1
        r["e_sum"] += e
        if r["e_min"] is None or e < r["e_min"]:
            r["e_min"], r["best"], r["ties"] = e, i, 1
        elif e == r["e_min"]:
            r["ties"] += 1
    for r in out:
        b = hits[r["best"]]
        assert b["bp_count"] == 2
        r["e_acc"], r["e_hyb"] = float(b["e_acc"]), float(b["e_hyb"])
        r["bp_first"] = bp[b["bp_offset"]].tolist()
        r["bp_last"] = bp[b["bp_offset"] + 1].tolist()
    return out


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_same(pairs, ref, what):
    assert len(pairs) == len(ref), (what, len(pairs), len(ref))
    for k, (p, r) in enumerate(zip(pairs, ref)):
        assert (int(p["query"]), int(p["db_id"]), int(p["hits"])) == (r["query"], r["db_id"], r["hits"]), (what, k)
        for f in ("e_min", "e_sum", "e_acc", "e_hyb"):
            assert bits(p[f]) == bits(r[f]), (what, k, f, float(p[f]), r[f])
        assert p["bp_first"].tolist() == r["bp_first"] and p["bp_last"].tolist() == r["bp_last"], (what, k)


def tie_case(ctx, tmp_path):
    """A target made of A and C only (no base pair inside it: every window is fully accessible) carrying one site
    twice in identical surroundings, and a query with its complement: the two hits of the pair have the same
    energy bit for bit."""
    from priblast_amd import capi
    site = "CCACCACACCCAACCACACC"
    comp = site[::-1].translate(str.maketrans("AC", "UG"))
    target = "C" * 30 + site + "C" * 30 + site + "C" * 30
    prefix = str(tmp_path / "tiedb")
    capi.db_build(ctx, prefix, ["tie_target", "decoy"], [target, "ACGU" * 25])
    return prefix, ["UUUUUUUUUU" + comp + "UUUUUUUUUU", "GGGAAACCCUUU" * 6]


def cases(ctx, golden_dir, tmp_path):
    for tag in ("c1", "mix", "quirk"):
        names, seqs = refdump.read_fasta(os.path.join(GOLDEN, f"{tag}_q.fa"))
        yield tag, os.path.join(golden_dir, f"{tag}db"), seqs
    prefix, seqs = tie_case(ctx, tmp_path)
    yield "tie", prefix, seqs


def summaries(ctx, prefix, seqs, opts, max_resident_pages=None):
    from priblast_amd import capi
    db = capi.Db(ctx, prefix, max_resident_pages)
    qb = capi.QBatch(ctx, seqs, db.repeat_flag)
    try:
        qb.accessibility(db.W, db.delta)
        return [capi.search_page_summary(ctx, qb, db, p, opts, with_counts=True) for p in range(db.npages)]
    finally:
        qb.close()
        db.close()


def test_summary_equals_reduced_hit_path(ctx, golden_dir, tmp_path):
    from priblast_amd import capi
    ties = total = 0
    for tag, prefix, seqs in cases(ctx, golden_dir, tmp_path):
        db = capi.Db(ctx, prefix)
        qb = capi.QBatch(ctx, seqs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        try:
            for kw in OPTS:
                for page in range(db.npages):
                    hits, bp, counts = capi.search_page(ctx, qb, db, page, capi.default_opts(output_style=0, **kw))
                    ref = reduce_hits(hits, bp)
                    pairs, pcounts = capi.search_page_summary(ctx, qb, db, page, capi.default_opts(output_style=0, **kw),
                                                              with_counts=True)
                    assert pcounts == counts
                    assert_same(pairs, ref, (tag, kw, page))
                    # -s has no effect on the records
                    assert np.array_equal(capi.search_page_summary(ctx, qb, db, page, capi.default_opts(output_style=1, **kw)), pairs)
                    ties += sum(r["ties"] > 1 for r in ref)
                    total += len(ref)
        finally:
            qb.close()
            db.close()
    assert total > 50
    assert ties > 0  # the first-minimum rule was exercised


@pytest.mark.parametrize("knob", ["PRB_SEARCH_PAIRS=1", "PRB_GAPPED_CHUNK_HITS=3", "PRB_TRACE_NO_SLOTS=1", "resident=1"])
def test_summary_invariance(ctx, golden_dir, monkeypatch, knob):
    """one sub-batch per query; the gapped stage in chunks of three hits; every final hit re-extended for its base
    pairs; the 3-page database streamed through one resident page: the same records"""
    from priblast_amd import capi
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    prefix = os.path.join(golden_dir, "mixdb")
    for kw in OPTS[:2]:
        opts = capi.default_opts(**kw)
        plain = summaries(ctx, prefix, seqs, opts)
        assert sum(len(p) for p, _ in plain) > 10
        name, value = knob.split("=")
        if name == "resident":
            other = summaries(ctx, prefix, seqs, opts, max_resident_pages=int(value))
        else:
            monkeypatch.setenv(name, value)
            other = summaries(ctx, prefix, seqs, opts)
            monkeypatch.delenv(name)
        for (a, ca), (b, cb) in zip(plain, other):
            assert ca[2] == cb[2]
            assert a.tobytes() == b.tobytes(), (knob, kw)


def test_summary_of_a_query_without_hits(ctx, golden_dir):
    pages = summaries(ctx, os.path.join(golden_dir, "mixdb"), ["A" * 60], None)
    assert len(pages) == 3
    for pairs, counts in pages:
        assert len(pairs) == 0 and counts[2] == 0


def run_ris(golden_dir, tmp_path, tag, name, extra=(), env_extra=None):
    from priblast_amd import capi
    out = str(tmp_path / name)
    env = dict(os.environ, PRB_BATCH="5", **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, f"{tag}_q.fa"), "-o", out, "-d",
                    os.path.join(golden_dir, f"{tag}db")] + list(extra), check=True, env=env)
    with open(out) as f:
        return f.read()


@pytest.mark.parametrize("tag", ["mix", "quirk"])
def test_cli_summary_matches_reference(golden_dir, tmp_path, tag):
    text = run_ris(golden_dir, tmp_path, tag, "sum.txt", ["-t"])
    full = run_ris(golden_dir, tmp_path, tag, "full.txt")
    lines, flines = text.splitlines(), full.splitlines()
    assert lines[:2] == flines[:2] and lines[2] == SUMMARY_COLUMNS
    body = [l.split(",") for l in lines[3:]]
    assert [int(f[0]) for f in body] == list(range(len(body)))
    assert all(len(f) == 11 for f in body)
    # the reference's result lines (sorted, without Id), per (query name, target name)
    with open(os.path.join(GOLDEN, f"{tag}_ris_s0.out")) as f:
        gold = f.read().splitlines()[2:]
    ref = defaultdict(list)
    for l in gold:
        f = l.split(",")
        ref[(f[0], f[2])].append(f)
    # this build's own full output, in its (deterministic) order
    own = defaultdict(list)
    for l in flines[3:]:
        f = l.split(",")[1:]
        own[(f[0], f[2])].append(f)
    got = {(f[1], f[3]): f for f in body}
    assert len(got) == len(body)  # one line per pair
    assert set(got) == set(ref)
    for key, f in got.items():
        g = ref[key]
        hits, emin, esum, eacc, ehyb, bpf = int(f[5]), f[6], float(f[7]), f[8], f[9], f[10]
        assert f[2] == g[0][1] and f[4] == g[0][3]  # lengths
        assert hits == len(g)
        lo = min(float(x[6]) for x in g)
        tied = [x for x in g if float(x[6]) == lo]
        assert emin == tied[0][6]
        if len(tied) == 1:
            assert (eacc, ehyb, bpf) == (tied[0][4], tied[0][5], tied[0][7])
        else:
            assert [eacc, ehyb, emin, bpf] in [x[4:8] for x in own[key]]
        assert abs(esum - sum(float(x[6]) for x in g)) <= 1e-4 * hits
    # two workers in one process write the same file
    assert run_ris(golden_dir, tmp_path, tag, "two.txt", ["-t"], {"PRB_DEVICES": "0,0"}) == text
    # -s has no effect
    assert run_ris(golden_dir, tmp_path, tag, "s1.txt", ["-t", "-s", "1"]) == text
