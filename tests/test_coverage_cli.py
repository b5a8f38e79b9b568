"""The refusals of `ris -c D` (the regions of each target bound by at least D queries), all before any GPU work: its row
of the switch table (not with -t, -n, -q, -k, -b, -r; not with one process per GPU; -u combines), the range of D, and the
usage text."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

C = "-c (the regions of each target bound by at least D queries)"
PARTNER = {
    "-t": "-t (per-pair summary lines)",
    "-n 3": "-n (the N best pairs per query)",
    "-q": "-q (per-position profile lines)",
    "-k 3": "-k (the N best interaction sites per query)",
    "-b": "-b (binary hit records)",
    "-r 3": "-r (the N best queries per target)",
}
C_RANGE = "Error: -c needs an integer between 1 and 1000000 (this build's limit)"
C_RANKS = "Error: " + C + " is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process"
MARKS = ("can't be combined with", " needs -", "needs an integer", "is not supported with one process per GPU")


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


@pytest.mark.parametrize("reverse", [False, True], ids=["c_first", "c_last"])
@pytest.mark.parametrize("partner", list(PARTNER))
def test_c_is_refused_with_the_other_output_switches(tmp_path, partner, reverse):
    groups = [["-c", "2"], partner.split()]
    extra = sum(groups[::-1] if reverse else groups, [])
    refused(tmp_path, ris(tmp_path, extra), f"Error: {C} can't be combined with {PARTNER[partner]}")


def test_c_takes_precedence_only_where_it_is_given(tmp_path):
    # -c with two partners: the row's partners from the first to the last; without -c the older rows answer as before
    refused(tmp_path, ris(tmp_path, ["-c", "2", "-r", "3", "-t"]), f"Error: {C} can't be combined with {PARTNER['-t']}")
    refused(tmp_path, ris(tmp_path, ["-r", "3", "-t"]),
            "Error: -r (the N best queries per target) can't be combined with -t (per-pair summary lines)")
    refused(tmp_path, ris(tmp_path, ["-k", "3", "-t"]),
            "Error: -k (the N best interaction sites per query) can't be combined with -t (per-pair summary lines)")
    refused(tmp_path, ris(tmp_path, ["-n", "3"]), "Error: -n (the N best pairs per query) needs -t (per-pair summary lines)")
    refused(tmp_path, ris(tmp_path, ["-r", "1025"]), "Error: -r needs an integer between 1 and 1024 (this build's limit)")


@pytest.mark.parametrize("value", ["0", "-1", "1000001", "abc", ""])
def test_c_needs_a_depth_in_range(tmp_path, value):
    refused(tmp_path, ris(tmp_path, ["-c", value]), C_RANGE)
    refused(tmp_path, ris(tmp_path, ["-u", "-c", value]), C_RANGE)


def test_c_is_refused_with_one_process_per_gpu(tmp_path):
    refused(tmp_path, ris(tmp_path, ["-c", "2"], ranks=True), C_RANKS)
    refused(tmp_path, ris(tmp_path, ["-c", "2", "-u"], ranks=True), C_RANKS)


def test_c_combines_with_u(tmp_path):
    for extra in (["-c", "2", "-u"], ["-u", "-c", "1000000"], ["-c", "1"]):
        r = ris(tmp_path, extra)  # (what follows depends on whether a device is present)
        assert not any(m in r.stderr for m in MARKS), r.stderr


def test_usage_names_c():
    from priblast_amd import capi
    text = subprocess.run([capi.BIN_PATH, "-h"], capture_output=True, text=True).stdout
    assert "    -c INT " in text and "distinct queries" in text
