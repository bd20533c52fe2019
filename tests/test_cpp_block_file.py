"""fileBlocks / readFile of the C++ IBlockDevice adapter (include/ppfs_gpu/block_device.hpp).

CPU: tests/cpp/test_block_file.cpp compiles and links against the engine library.  GPU: the program compares
each call with the default per-block loop (the read-only BlockIndexIterator walk through readBlock) on a copy
of the disk -- result, blocks or bytes, disk image, correction log in order; for a case with a failing block
the result and everything up to that block -- for each codec on StackDisk, MappedFileDisk and an unmapped
disk."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "paritypartyfs_amd", "_lib")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libppfs_ecc.so")):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    out = str(tmp_path_factory.mktemp("block_file") / "test_block_file")
    src = os.path.join(ROOT, "tests", "cpp", "test_block_file.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-parameter",
                        "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + LIBDIR, "-lppfs_ecc",
                        "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cpp_block_file_builds(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_file_calls_equal_the_per_block_loop(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
