"""CPU checks of the inode reads (include/ppfs_ecc.h ppfs_ecc_inode_span, ppfs_ecc_read_inodes_*): the arithmetic and
the status rule (csrc/inode_plan.hpp, tests/cpp/test_inode_plan.cpp) under the address and undefined-behaviour
sanitizers, the new ABI without a GPU, and the new kernels' code-object resources.  What needs a context -- the reads
themselves, and ppfs_ecc_inode_span against the closed form -- is in tests/test_gpu_inodes.py: a context cannot be
made without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_inode_span", "ppfs_ecc_read_inodes_device", "ppfs_ecc_read_inodes_host")
KERNELS = ("inode_bitmap_extents_kernel", "inode_table_extents_kernel", "inode_status_kernelINS_10ReadPiecesE")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inode_plan") / "test_inode_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_inode_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_inode_plan(plan_exe):
    """For ds in {1, 2, 3, 27, 31, 79, 80, 81, 82, 162, 249, 4091, 4095, 65535}: every inode of a table of ds + 300
    inodes and the 256 numbers below 2^32 (with table and bitmap blocks that carry the block number past 32 bits)
    against a literal restatement of _getInodeLocation, _readInode's two-branch loop over a clamping readBlock and
    Bitmap::_getByteLocation / getBit; pieces <= K(ds), with equality where gcd(81, ds) = 1; the device call's piece;
    the status rule against InodeManager::get's order of evaluation over all status combinations of inodes of one to
    three pieces and random ones of an inode of 81; the shared epilogue (bitmap_step, inode_status) for K in {2, 3, 4,
    81} against a restatement of its four former copies, final status and the piece_status row in a heap buffer of
    exactly 1 + K bytes, over every bitmap state and the same piece statuses; slot_of and the read's extents against
    piece(); the row split over a heap buffer of exactly 81 bytes."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_inode_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native, ecc
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\((const )?ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    for method in ("inode_span", "read_inodes", "read_inodes_host"):
        assert callable(getattr(EccEngine, method))
    assert ecc.INODE_TABLE_DTYPE is _native.INODE_TABLE_DTYPE and ecc.INODE_META_DTYPE is _native.INODE_META_DTYPE
    assert ecc.InodeCounts._fields[:5] == ("ok", "corrected", "failed", "out_of_range", "not_allocated")
    assert _native.INODE_TABLE_DTYPE.itemsize == 16 and _native.INODE_META_DTYPE.itemsize == 24
    assert ctypes.sizeof(_native.InodeCounts) == 64 and len(ecc.InodeCounts._fields) == 8
    piece = re.search(r"^#define PPFS_ECC_INODE_PIECE (\d+)$", header, flags=re.M)
    assert piece and int(piece.group(1)) == _native.INODE_PIECE
    plan = open(os.path.join(ROOT, "paritypartyfs_amd", "csrc", "inode_plan.hpp")).read()
    assert re.search(rf"PIECE_INODES = {_native.INODE_PIECE};", plan)
    # the structs of the header, field by field, against the dtypes and the ctypes record
    width = {"uint64_t": 8, "uint32_t": 4, "uint8_t": 1}

    def fields(struct):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            m = re.match(r"\s*(uint64_t|uint32_t|uint8_t)\s+(.*)", decl.strip(), flags=re.S)
            if m:
                for name, dim in re.findall(r"(\w+)(?:\[(\d+)\])?", m.group(2)):
                    out.append((name, width[m.group(1)] * int(dim or 1)))
        return out

    table = fields("ppfs_ecc_inode_table")
    assert [n for n, _ in table] == list(_native.INODE_TABLE_DTYPE.names) and sum(b for _, b in table) == 16
    meta = fields("ppfs_ecc_inode_meta")
    assert [n for n, _ in meta] == list(_native.INODE_META_DTYPE.names) and sum(b for _, b in meta) == 24
    assert [(n, _native.INODE_META_DTYPE.fields[n][1]) for n, _ in meta] == [("time_creation", 0), ("time_modified", 8),
                                                                             ("type", 16), ("pad", 17)]
    counts = fields("ppfs_ecc_inode_counts")
    assert sum(b for _, b in counts) == 64
    assert [n for n, _ in counts][:5] == [n for n, _ in _native.InodeCounts._fields_][:5]


def test_inode_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(128)
    table = np.zeros(1, _native.INODE_TABLE_DTYPE)
    table["total_inodes"] = 10
    a = ctypes.c_uint32()
    assert lib.ppfs_ecc_inode_span(None, table.ctypes.data, 1, ctypes.byref(a), None, None) == -22
    assert lib.ppfs_ecc_read_inodes_device(None, buf, 1, table.ctypes.data, buf, 4, 1, None, None, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_read_inodes_host(None, buf, 1, table.ctypes.data, buf, 4, 1, None, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_read_inodes_host(None, buf, 1, table.ctypes.data, buf, 4, 0, None, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_inode_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
            assert 0 < d["vgpr_count"] <= 64, (n, d)  # at most 64 VGPRs: 8 waves per SIMD
