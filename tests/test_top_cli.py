"""The refusals of `ris -t -n N` (the N best pairs per query), which come before any GPU work."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def ris(tmp_path, extra, env_extra=None):
    from priblast_amd import capi
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"),
                           "-d", str(tmp_path / "nodb")] + extra, capture_output=True, text=True, env=env)


@pytest.mark.parametrize("extra", [["-n", "3"], ["-n", "3", "-s", "1"]])
def test_top_needs_summary_lines(tmp_path, extra):
    r = ris(tmp_path, extra)
    assert r.returncode != 0 and "-n" in r.stderr and "-t" in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("n", ["0", "-1", "1025", "100000", "abc", "3x", ""])
def test_top_refuses_n_out_of_range(tmp_path, n):
    r = ris(tmp_path, ["-t", "-n", n])
    assert r.returncode != 0 and "-n" in r.stderr
    assert not (tmp_path / "out").exists()


def test_top_refuses_binary_output(tmp_path):
    # the refusal of -t -b, with its message
    r = ris(tmp_path, ["-t", "-n", "3", "-b"])
    assert r.returncode != 0 and "-t" in r.stderr and "-b" in r.stderr
    assert not (tmp_path / "out").exists()
    r = ris(tmp_path, ["-n", "3", "-b"])
    assert r.returncode != 0 and "-n" in r.stderr
    assert not (tmp_path / "out").exists()


def test_top_refuses_rank_mode(tmp_path):
    r = ris(tmp_path, ["-t", "-n", "3"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "-t" in r.stderr and "WORLD_SIZE" in r.stderr
    assert not (tmp_path / "out").exists()


def test_usage_names_the_top_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -n " in r.stdout
