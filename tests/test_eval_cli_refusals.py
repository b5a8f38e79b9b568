"""The refusals of `ris -E`, pinned as tests/test_cli_refusals.py pins those of the older switches: first lines of
stderr, no output file, no device needed - they come before any GPU work.  `-E` needs -k, goes with none of -b -t -n -q
-r -c -z -G -P nor with one process per GPU, takes 1..100000, and is one of the three switches that `-Z` goes with."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

E = "-E (an E-value and a q-value per interaction site from N pooled decoys per query)"
K = "-k (the N best interaction sites per query)"
WITH = {
    "-b": "-b (binary hit records)",
    "-t": "-t (per-pair summary lines)",
    "-q": "-q (per-position profile lines)",
    "-r 3": "-r (the N best queries per target)",
    "-c 2": "-c (the regions of each target bound by at least D queries)",
    "-t -z 4": "-t (per-pair summary lines)",   # (a row's partners from the first to the last: -t comes before -z)
    "-z 4": "-z (an empirical p-value per pair from N shuffled decoys)",
    "-t -G groups.tsv": "-t (per-pair summary lines)",
    "-G groups.tsv": "-G (one line per query-group pair)",
    "-P 4": "-P (an empirical p-value per query-group pair from N shuffled decoys)",
}
RANGE = "Error: -E needs an integer between 1 and 100000 (this build's limit)"
RANKS = f"Error: {E} is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
MARKS = ("can't be combined with", " needs -", "needs an integer", "needs a non-negative integer", "is not supported with one process per GPU")


def ris(tmp_path, extra, ranks=False):
    from priblast_amd import capi
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    if ranks:
        env.update(WORLD_SIZE="2", RANK="0")
    return subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"),
                           "-d", str(tmp_path / "nodb")] + extra, capture_output=True, text=True, env=env)


def refused(tmp_path, r, want):
    assert (r.stderr.splitlines() or [""])[0] == want
    assert r.returncode != 0
    assert not (tmp_path / "out").exists()


def test_e_needs_k(tmp_path):
    refused(tmp_path, ris(tmp_path, ["-E", "3"]), f"Error: {E} needs {K}")
    refused(tmp_path, ris(tmp_path, ["-E", "3", "-u"]), f"Error: {E} needs {K}")


@pytest.mark.parametrize("reverse", [False, True], ids=["as_given", "reversed"])
@pytest.mark.parametrize("other", list(WITH))
def test_e_goes_with_none_of_the_other_output_switches(tmp_path, other, reverse):
    groups = [["-k", "5"], ["-E", "3"], other.split()]
    extra = sum(groups[::-1] if reverse else groups, [])
    refused(tmp_path, ris(tmp_path, extra), f"Error: {E} can't be combined with {WITH[other]}")


@pytest.mark.parametrize("value", ["0", "100001", "abc", "-1"])
def test_the_range_of_e(tmp_path, value):
    refused(tmp_path, ris(tmp_path, ["-k", "5", "-E", value]), RANGE)
    # ... after the combinations, before nothing else of -E
    refused(tmp_path, ris(tmp_path, ["-k", "5", "-E", value, "-b"]), f"Error: {E} can't be combined with {WITH['-b']}")


def test_the_seed_goes_with_e_alone(tmp_path):
    for extra in (["-k", "5", "-E", "3", "-Z", "7"], ["-k", "5", "-E", "100000"], ["-k", "5", "-E", "1", "-u", "-s", "1"]):
        r = ris(tmp_path, extra)   # accepted: what follows depends on whether a device is present
        assert not any(m in r.stderr for m in MARKS), r.stderr
    refused(tmp_path, ris(tmp_path, ["-k", "5", "-E", "3", "-Z", "x"]), "Error: -Z needs a non-negative integer")
    # (without a switch that makes decoys -Z is refused as before)
    refused(tmp_path, ris(tmp_path, ["-k", "5", "-Z", "7"]),
            "Error: -Z (the seed of the decoys' shuffles) needs -z (an empirical p-value per pair from N shuffled decoys)")


def test_e_is_refused_with_one_process_per_gpu(tmp_path):
    refused(tmp_path, ris(tmp_path, ["-k", "5", "-E", "3"], ranks=True), RANKS)
    refused(tmp_path, ris(tmp_path, ["-E", "3", "-Z", "1", "-k", "5"], ranks=True), RANKS)
