"""The host path's arithmetic and CPU copies (paritypartyfs_amd/csrc/host_plan.hpp, host_copy.hpp) on
the host: chunk sizes of a call (no piece beyond the staging layout, the default sequences as they
were), the staging layout, the changed-block scan, the patch-list application and the threaded
copies (tests/cpp/test_host_plan.cpp).  CPU only: g++ builds it, without HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan") / "test_host_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_host_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", src, "-o", out, "-pthread"], check=True)
    return out


def _run(exe, args=(), **env):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def test_host_plan(exe):
    _run(exe)


@pytest.mark.parametrize("env", [{"PPFS_ECC_COPY_NT": "0"}, {"PPFS_ECC_COPY_THREADS": "1"}],
                         ids=["plain-memcpy", "single-thread"])
def test_host_copies_other_modes(exe, env):
    out = _run(exe, ("copies",), **env)
    if "PPFS_ECC_COPY_THREADS" in env:
        assert "copy threads 1" in out
