"""lookupNames / lookupInodes of the C++ IBlockDevice adapter (include/ppfs_gpu/block_device.hpp).

CPU: tests/cpp/test_block_lookup.cpp compiles and links against the engine library.  GPU: the program compares one
lookupNames / lookupInodes call with IBlockDevice::lookup_loop, the loop of DirectoryManager::getInodeByName that is its
definition, on a copy of the disk -- per query the result, the error, the inode and the entry, then the disk image and
the correction log under the adapter contract (the loop's events first and in order, then the blocks corrected beyond
the loop's reach; the disk the loop's with exactly those blocks corrected as well), with a corrected index block, a
corrected data block and a failing data block that has a correctable one behind it -- for each codec on StackDisk,
MappedFileDisk and an unmapped disk."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "paritypartyfs_amd", "_lib")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libppfs_ecc.so")):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    out = str(tmp_path_factory.mktemp("block_lookup") / "test_block_lookup")
    src = os.path.join(ROOT, "tests", "cpp", "test_block_lookup.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-parameter",
                        "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + LIBDIR, "-lppfs_ecc",
                        "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cpp_block_lookup_builds(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_lookup_equals_the_loop(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
