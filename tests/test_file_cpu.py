"""CPU checks of the read-only file walk (include/ppfs_ecc.h ppfs_ecc_file_span, ppfs_ecc_file_tree_blocks,
ppfs_ecc_file_blocks_*, ppfs_ecc_read_file_*): the tree arithmetic (csrc/file_plan.hpp,
tests/cpp/test_file_plan.cpp) under the address and undefined-behaviour sanitizers, the new ABI without a GPU,
and the new kernels' code-object resources.  What needs a context (the span and tree-block values, ranges past
the file or the tree) is in tests/test_gpu_file.py: a context cannot be made without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_file_span", "ppfs_ecc_file_tree_blocks", "ppfs_ecc_file_blocks_device", "ppfs_ecc_file_blocks_host",
         "ppfs_ecc_read_file_device", "ppfs_ecc_read_file_host")
KERNELS = ("files_expand_kernelINS_7OneFileE", "files_extents_kernelINS_7OneFileE", "files_merge_kernelINS_7OneFileE")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("file_plan") / "test_file_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_file_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_file_plan(plan_exe):
    """path_of against a step-by-step iterator for every block up to the capacity, ipb 0, 1, 2, 3, 14, 62; for
    ipb <= 3 and every (first, count) up to the capacity the per-level tree counts, the parent / slot relations and
    the first block under each tree entry against brute force; span's clamps and the closed-form extents against
    extent_plan.hpp's file_extents; the expansion over heap buffers of exactly the scratch's size, with index blocks
    of status 1, 5 and 9 at each level."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_file_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.ecc import FILE_COUNT_FIELDS, EccEngine, FileCounts

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^(int|long long) {name}\((const )?ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    for method in ("file_span", "file_tree_blocks", "file_blocks", "file_blocks_host", "read_file", "read_file_host"):
        assert callable(getattr(EccEngine, method))
    assert _native.FILE_DTYPE.itemsize == 64 and ctypes.sizeof(_native.FileCounts) == 64
    assert FileCounts._fields == FILE_COUNT_FIELDS == tuple(f for f, _ in _native.FileCounts._fields_)
    for struct, fields in (("ppfs_ecc_file", list(_native.FILE_DTYPE.names)), ("ppfs_ecc_file_counts", list(FILE_COUNT_FIELDS))):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(?!uint64_t\b|uint32_t\b)(\w+)(?:\[\d+\])?\s*[,;]", body) == fields
    f = np.zeros(1, _native.FILE_DTYPE)
    f["direct"][0, 11], f["indirect"], f["file_size"] = 7, 8, 9
    assert f.view("<u4").tolist() == [0] * 11 + [7, 8, 0, 0, 9]  # the record as sixteen dwords


def test_file_calls_of_a_null_context_or_file_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)
    assert lib.ppfs_ecc_file_span(None, buf, 0, 1, None, None, None) == -22
    assert lib.ppfs_ecc_file_tree_blocks(None, buf, 0, 1) == -22
    assert lib.ppfs_ecc_file_blocks_device(None, buf, 1, buf, 0, 1, None, None, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_file_blocks_host(None, buf, 1, buf, 0, 1, None, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_read_file_device(None, buf, 1, buf, 0, 1, buf, 1, None, None, 1, None) == -22
    assert lib.ppfs_ecc_read_file_host(None, buf, 1, buf, 0, 1, buf, 1, None, None, 1) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_file_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
