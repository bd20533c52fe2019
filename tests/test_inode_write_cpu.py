"""CPU checks of the inode writes (include/ppfs_ecc.h ppfs_ecc_write_inodes_*): the grouping step (csrc/inode_wplan.hpp,
tests/cpp/test_inode_wplan.cpp) under the address and undefined-behaviour sanitizers, the new ABI without a GPU, and
the new kernels' code-object resources.  The writes themselves need a context, which cannot be made without a GPU:
tests/test_gpu_inode_write.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_write_inodes_device", "ppfs_ecc_write_inodes_host")
KERNELS = ("inode_elect_kernel", "inode_owner_extents_kernel", "inode_overlay_kernel", "inode_status_kernelINS_11WritePiecesE")


@pytest.fixture(scope="module")
def wplan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inode_wplan") / "test_inode_wplan")
    src = os.path.join(ROOT, "tests", "cpp", "test_inode_wplan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_inode_wplan(wplan_exe):
    """For ds in {1, 31, 79, 80, 81, 249, 4091} and full pieces of distinct, consecutive, repeated and one repeated
    inode number: the election the kernels run, serially in shuffled orders, against brute force -- the owner of every
    block is its lowest slot, the winner of every number its highest entry, every probe ends within the capacity, one
    extent per distinct block, every touched byte written once with the loop's bytes, the composed row is the packed
    Inode, and the host form's hulls cover exactly the touched bytes."""
    r = subprocess.run([wplan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    longest = int(re.search(r"longest probe sequence: (\d+)", r.stdout).group(1))
    assert 1 <= longest <= 65536  # the largest capacity


def test_inode_write_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.block_device import IBlockDevice
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    # the mirror of the reads: the same arguments, files and meta const
    for form in ("device", "host"):
        read = re.search(rf"^int ppfs_ecc_read_inodes_{form}\((.*?)\);", header, flags=re.M | re.S).group(1)
        write = re.search(rf"^int ppfs_ecc_write_inodes_{form}\((.*?)\);", header, flags=re.M | re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s)
        expect = norm(read).replace("ppfs_ecc_file* ", "const ppfs_ecc_file* ").replace("ppfs_ecc_inode_meta* ", "const ppfs_ecc_inode_meta* ")
        assert norm(write) == expect, form
    for method in ("write_inodes", "write_inodes_host"):
        assert callable(getattr(EccEngine, method))
    assert callable(IBlockDevice.write_inodes)
    block_device = open(os.path.join(ROOT, "include", "ppfs_gpu", "block_device.hpp")).read()
    assert "writeInodes" in block_device


def test_inode_write_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(128)
    table = np.zeros(1, _native.INODE_TABLE_DTYPE)
    table["total_inodes"] = 10
    t = table.ctypes.data
    assert lib.ppfs_ecc_write_inodes_device(None, buf, 1, t, buf, 4, 1, buf, buf, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_write_inodes_host(None, buf, 1, t, buf, 4, 1, buf, buf, None, None, None, 1) == -22
    assert lib.ppfs_ecc_write_inodes_host(None, buf, 1, t, buf, 4, 0, None, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_inode_write_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
            assert 0 < d["vgpr_count"] <= 64, (n, d)  # at most 64 VGPRs: 8 waves per SIMD
