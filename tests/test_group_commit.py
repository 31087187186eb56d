"""The group-commit queue of the shared calls (fedtree_amd/csrc/group_commit.hpp) without a GPU:
tools/group_commit_test.cpp drives it with a fake runner -- every caller its own result, one leader at a time
per queue, a throwing batch fails alone and blocks nobody, a lone caller never lingers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("group_commit") / "group_commit_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "group_commit_test.cpp"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("linger", [None, "0"])
def test_group_commit_protocol(exe, linger):
    env = {k: v for k, v in os.environ.items() if k != "FTHE_LINGER_US"}
    if linger is not None:
        env["FTHE_LINGER_US"] = linger
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    want = f"group commit OK (FTHE_LINGER_US={linger or 200})"
    assert r.returncode == 0 and want in r.stdout, r.stdout + r.stderr
