"""CPU checks of the file writes (include/ppfs_ecc.h ppfs_ecc_write_file_*, ppfs_ecc_write_files_*): the write side of
the batch arithmetic (csrc/files_plan.hpp, tests/cpp/test_files_write_plan.cpp) under the address and
undefined-behaviour sanitizers, the new ABI and its refusals without a GPU, the block devices' per-block loops, and the
new kernels' code-object resources.  What needs a context is in tests/test_gpu_file_write.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_write_file_device", "ppfs_ecc_write_file_host", "ppfs_ecc_write_files_device", "ppfs_ecc_write_files_host")
KERNELS = ("files_written_init_kernelINS_7OneFileE", "files_write_merge_kernelINS_7OneFileE", "files_written_init_kernelINS_5BatchE",
           "files_write_merge_kernelINS_5BatchE")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("files_write_plan") / "test_files_write_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_files_write_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_files_write_plan(plan_exe):
    """For ds 58, 2, 16 and 508: the strict range rule (one byte past the end, an offset at the end, an overflowing
    sum, the number of the file refused) and the repeat detector against brute force over all pairs -- identical
    records with touching, intersecting and disjoint spans, different records with equal spans, empty ranges, a later
    pair hidden behind a long early span, 3,000 seeded batches per size; an accepted batch's slots are the read plan's."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_write_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.block_device import IBlockDevice
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(ppfs_ecc_ctx\* ctx, const uint8_t\* (d_)?in, size_t in_bytes,", header, flags=re.M), name
    for method in ("write_file", "write_file_host", "write_files", "write_files_host"):
        assert callable(getattr(EccEngine, method))
    assert callable(IBlockDevice.write_file) and callable(IBlockDevice.write_files)
    assert "file_io.cpp:46-104" in header


def test_write_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(128)
    assert lib.ppfs_ecc_write_file_device(None, buf, 1, buf, 1, buf, 0, 1, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_write_file_host(None, buf, 1, buf, 1, buf, 0, 1, None, None, None, 1) == -22
    assert lib.ppfs_ecc_write_files_device(None, buf, 1, buf, 1, buf, None, 1, None, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_write_files_host(None, buf, 1, buf, 1, buf, None, 1, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_the_per_block_loop_of_a_raw_device():
    """IBlockDevice.write_file / write_files on a device without a codec: direct blocks only need no engine."""
    from paritypartyfs_amd._native import FILE_DTYPE
    from paritypartyfs_amd.block_device import ECCType, FsError, HeapDisk, create_block_device

    bs, blocks = 16, 12
    disk = HeapDisk(bs * blocks)
    disk.buf[:] = 0xEE
    dev = create_block_device(disk, bs, ECCType(0))
    f = np.zeros(1, FILE_DTYPE)
    f["direct"][0] = [7, 3, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    f["file_size"] = 3 * bs + 5
    data = bytes(range(1, 30))
    assert dev.write_file(f, 10, data) == (29, None)
    img = disk.buf.reshape(blocks, bs)
    assert bytes(img[7, 10:]) == data[:6] and bytes(img[3]) == data[6:22] and bytes(img[9, :7]) == data[22:]
    assert (img[7, :10] == 0xEE).all() and (img[9, 7:] == 0xEE).all() and (img[1] == 0xEE).all()
    before = disk.buf.copy()
    assert dev.write_file(f, 3 * bs, b"x" * 6) == (0, FsError.FileIO_OutOfBounds)  # one byte past file_size: nothing grows
    assert dev.write_file(f, 3, b"") == (0, None)
    assert np.array_equal(disk.buf, before)
    got = dev.write_files(np.concatenate([f, f]), [(0, 2), (3 * bs + 4, 1)], [b"ab", b"c"])
    assert got == [(2, None), (1, None)] and bytes(img[7, :2]) == b"ab" and img[1, 4] == ord("c")


def test_write_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
