"""CPU checks of the walk over a batch of files (include/ppfs_ecc.h ppfs_ecc_files_plan, ppfs_ecc_files_blocks_*,
ppfs_ecc_read_files_*): the batch arithmetic (csrc/files_plan.hpp, tests/cpp/test_files_plan.cpp) under the address
and undefined-behaviour sanitizers, the new ABI without a GPU, and the new kernels' code-object resources.  What
needs a context is in tests/test_gpu_files.py: a context cannot be made without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_files_plan", "ppfs_ecc_files_blocks_device", "ppfs_ecc_files_blocks_host", "ppfs_ecc_read_files_device",
         "ppfs_ecc_read_files_host")
KERNELS = ("files_expand_kernelINS_5BatchE", "files_extents_kernelINS_5BatchE", "files_merge_kernelINS_5BatchE")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("files_plan") / "test_files_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_files_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_files_plan(plan_exe):
    """For ipb 0, 1, 2, 3, 14 and batches of 1-6 files that between them take every (first, count) shape of the small
    trees, with empty files and runs of them: slots, totals, scratch positions and row tables against a per-file loop
    of the single-file plan; row_of for every entry; no window of 256 entries spans more than 256 rows; the merged
    expansion over heap buffers of exactly the scratch's size against the single-file expand run per file, with index
    blocks of status 1, 5 and 9; the refusals and the number of the file they name."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_files_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\((const )?ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    for method in ("files_plan", "files_blocks", "files_blocks_host", "read_files", "read_files_host"):
        assert callable(getattr(EccEngine, method))
    assert _native.FILES_SLOT_DTYPE.itemsize == 88 and _native.FILES_TOTALS_DTYPE.itemsize == 48
    for struct, dtype in (("ppfs_ecc_files_slot", _native.FILES_SLOT_DTYPE), ("ppfs_ecc_files_totals", _native.FILES_TOTALS_DTYPE),
                          ("ppfs_ecc_file_range", np.dtype([("offset", "<u8"), ("nbytes", "<u8")]))):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\b(?!uint64_t\b)(\w+)(\[\d+\])?\s*[,;]", body)
        assert [f for f, _ in fields] == list(dtype.names), struct
        assert sum(8 * (int(dim[1:-1]) if dim else 1) for _, dim in fields) == dtype.itemsize, struct


def test_files_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(128)
    assert lib.ppfs_ecc_files_plan(None, buf, None, 1, None, None) == -22
    assert lib.ppfs_ecc_files_blocks_device(None, buf, 1, buf, None, 1, None, None, None, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_files_blocks_host(None, buf, 1, buf, None, 1, None, None, None, None, None, None, 1) == -22
    assert lib.ppfs_ecc_read_files_device(None, buf, 1, buf, None, 1, buf, 1, None, None, None, 1, None) == -22
    assert lib.ppfs_ecc_read_files_host(None, buf, 1, buf, None, 1, buf, 1, None, None, None, 1) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_files_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
