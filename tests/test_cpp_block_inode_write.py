"""writeInodes of the C++ IBlockDevice adapter (include/ppfs_gpu/block_device.hpp).

CPU: tests/cpp/test_block_inode_write.cpp compiles and links against the engine library.  GPU: the program compares
one writeInodes call with IBlockDevice::writeInodes, the per-inode loop that is its definition, on a copy of the disk
-- per inode the error, then the disk image and the correction log in order and the inodes read back, with a
corrected bitmap block, a corrected table block that several inodes share and a failing table block in mid-batch --
for each codec on StackDisk, MappedFileDisk and an unmapped disk."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "paritypartyfs_amd", "_lib")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libppfs_ecc.so")):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    out = str(tmp_path_factory.mktemp("block_inode_write") / "test_block_inode_write")
    src = os.path.join(ROOT, "tests", "cpp", "test_block_inode_write.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-parameter",
                        "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + LIBDIR, "-lppfs_ecc",
                        "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cpp_block_inode_write_builds(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_write_inodes_equals_the_per_inode_loop(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
