"""The refusals of `ris -t` (per-pair summary lines), which come before any GPU work."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def ris(tmp_path, extra, env_extra=None):
    from priblast_amd import capi
    env = dict(os.environ, **(env_extra or {}))
    return subprocess.run([capi.BIN_PATH, "ris", "-i", os.path.join(GOLDEN, "mix_q.fa"), "-o", str(tmp_path / "out"),
                           "-d", str(tmp_path / "nodb")] + extra, capture_output=True, text=True, env=env)


def test_summary_refuses_binary_output(tmp_path):
    r = ris(tmp_path, ["-t", "-b"])
    assert r.returncode != 0 and "-t" in r.stderr and "-b" in r.stderr
    assert not (tmp_path / "out").exists()


def test_summary_refuses_rank_mode(tmp_path):
    r = ris(tmp_path, ["-t"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "-t" in r.stderr and "WORLD_SIZE" in r.stderr
    assert not (tmp_path / "out").exists()


def test_usage_names_the_summary_switch():
    from priblast_amd import capi
    r = subprocess.run([capi.BIN_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "\n    -t " in r.stdout
