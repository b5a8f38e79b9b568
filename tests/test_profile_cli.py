"""The refusals of `ris -q` (the per-position profile), which come before any GPU work."""
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


@pytest.mark.parametrize("extra,clash", [(["-q", "-t"], "-t"), (["-t", "-q"], "-t"), (["-q", "-n", "3"], "-n"),
                                         (["-q", "-t", "-n", "3"], "-t"), (["-q", "-b"], "-b")])
def test_profile_refuses_other_modes(tmp_path, extra, clash):
    r = ris(tmp_path, extra)
    assert r.returncode != 0 and "-q" in r.stderr and clash in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("env", [{"WORLD_SIZE": "2", "RANK": "0"}, {"PRB_FORCE_COMM": "1"}])
def test_profile_refuses_rank_mode(tmp_path, env):
    r = ris(tmp_path, ["-q"], env)
    assert r.returncode != 0 and "-q" in r.stderr and "WORLD_SIZE" in r.stderr
    assert not (tmp_path / "out").exists()


def test_usage_names_the_profile_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -q " in r.stdout
