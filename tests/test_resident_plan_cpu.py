"""The resident-prefix plan of the RS 2t <= 8 ticket launches (paritypartyfs_amd/csrc/resident_plan.hpp)
on the host: a zero-tile batch, a batch smaller and one larger than the prefix, override 0, fractional
and malformed PPFS_ECC_RESIDENT_MIB values (tests/cpp/test_resident_plan.cpp).  CPU only: g++ builds it
under the address and undefined-behaviour sanitizers, without HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resident_plan") / "test_resident_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_resident_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_resident_plan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
