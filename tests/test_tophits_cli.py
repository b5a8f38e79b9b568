"""The refusals of `ris -k N` (the N best interaction sites per query), which come before any GPU work."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def ris(tmp_path, extra, env_extra=None):
    from priblast_amd import capi
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRB_FORCE_COMM"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"),
                           "-d", str(tmp_path / "nodb")] + extra, capture_output=True, text=True, env=env)


@pytest.mark.parametrize("n", ["0", "-1", "1025", "100000", "abc", "3x", ""])
def test_tophits_refuses_n_out_of_range(tmp_path, n):
    r = ris(tmp_path, ["-k", n])
    assert r.returncode != 0 and "-k" in r.stderr and "1024" in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("extra,other", [(["-t"], "-t"), (["-t", "-n", "3"], "-t"), (["-n", "3"], "-n"), (["-q"], "-q")])
def test_tophits_refuses_the_other_reductions(tmp_path, extra, other):
    for args in (["-k", "3"] + extra, extra + ["-k", "3"]):
        r = ris(tmp_path, args)
        assert r.returncode != 0 and "-k" in r.stderr and other in r.stderr
        assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("env", [{"WORLD_SIZE": "2", "RANK": "0"}, {"PRB_FORCE_COMM": "1"}])
def test_tophits_refuses_rank_mode(tmp_path, env):
    r = ris(tmp_path, ["-k", "3"], env)
    assert r.returncode != 0 and "-k" in r.stderr and "WORLD_SIZE" in r.stderr
    assert not (tmp_path / "out").exists()


def test_usage_names_the_tophits_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -k " in r.stdout
