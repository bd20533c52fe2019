"""CPU checks of the allocated-block and list scrub (include/ppfs_ecc.h ppfs_ecc_scrub_allocated_*,
ppfs_ecc_scrub_list_*): the bitmap arithmetic (csrc/alloc_plan.hpp, tests/cpp/test_alloc_plan.cpp) under the
address and undefined-behaviour sanitizers, the new ABI without a GPU, and the new kernels' code-object
resources."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_scrub_list_device", "ppfs_ecc_scrub_list_host", "ppfs_ecc_scrub_allocated_device",
         "ppfs_ecc_scrub_allocated_host")
KERNELS = ("alloc_count_kernel", "alloc_offsets_kernel", "alloc_expand_kernel", "alloc_iota_kernel", "scrub_tally_kernel")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("alloc_plan") / "test_alloc_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_alloc_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_alloc_plan(plan_exe):
    """dataSize() 1, 3, 58, 249, 4080 x 13 bit counts around byte, word, bitmap-block and chunk boundaries x
    all-zero, all-one, alternating and random bitmaps x each bitmap block in turn failed, and a range of two
    pieces: word transform, masks, blocks spanned and the emulated count / offsets / expand equal a bit-by-bit
    restatement of Bitmap::getBit, and no read leaves the B * dataSize() stream."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_scrub_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    assert re.search(r"^#define PPFS_ECC_NOT_ALLOCATED 255\b", header, flags=re.M)
    assert _native.STATUS_NOT_ALLOCATED == 255
    for method in ("scrub_list", "scrub_list_host", "scrub_allocated", "scrub_allocated_host"):
        assert callable(getattr(EccEngine, method))
    assert ctypes.sizeof(_native.ScrubCounts) == 64
    fields = re.search(r"typedef struct ppfs_ecc_scrub_counts \{(.*?)\} ppfs_ecc_scrub_counts;", header, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"\b(?!uint64_t\b)(\w+)\s*[,;]", fields) == [f for f, _ in _native.ScrubCounts._fields_]


def test_scrub_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)
    assert lib.ppfs_ecc_scrub_list_device(None, buf, 1, buf, 1, None, None, None) == -22
    assert lib.ppfs_ecc_scrub_list_host(None, buf, 1, buf, 1, None, None) == -22
    assert lib.ppfs_ecc_scrub_allocated_device(None, buf, 1, 0, 0, 1, None, None, None, None) == -22
    assert lib.ppfs_ecc_scrub_allocated_host(None, buf, 1, 0, 0, 1, None, None, None) == -22
    assert lib.ppfs_ecc_last_error()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_scan_and_tally_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
