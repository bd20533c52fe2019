"""CPU checks of the direct list encode (paritypartyfs_amd/csrc/rs_wg_list.hpp rs_wg_encode_list_kernel;
include/ppfs_ecc.h ppfs_ecc_list_encode_kernel_name): the emission's store plan (csrc/list_store.hpp,
tests/cpp/test_list_store.cpp) under the address and undefined-behaviour sanitizers, the new ABI query
without a GPU, and the kernels' code-object resources."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import kernel_descriptors
from tests.test_list_direct_cpu import _group_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")


@pytest.fixture(scope="module")
def store_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("list_store") / "test_list_store")
    src = os.path.join(ROOT, "tests", "cpp", "test_list_store.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_list_store_plan(store_exe):
    """Every image alignment 0..15; images of 1, 2 and 70 blocks; lists of 1, 63, 64 and 65 entries with
    block 0, the last block, adjacent blocks and out-of-range entries: every byte of a listed row is
    written exactly once with its codeword byte, no other byte is written, every store is naturally
    aligned (the 16-byte ones 16-byte aligned) and inside the image."""
    r = subprocess.run([store_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_list_encode_kernel_name_is_part_of_the_abi():
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.ecc import EccEngine

    assert "ppfs_ecc_list_encode_kernel_name" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    assert re.search(r"^const char\* ppfs_ecc_list_encode_kernel_name\(const ppfs_ecc_ctx\* ctx\);", header, flags=re.M)
    assert callable(EccEngine.list_encode_kernel_name)


def test_list_encode_kernel_name_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    assert lib.ppfs_ecc_list_encode_kernel_name.restype is ctypes.c_char_p
    assert lib.ppfs_ecc_list_encode_kernel_name(None) == b""
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    assert re.search(r"\bT ppfs_ecc_list_encode_kernel_name$", out, flags=re.M)


def test_list_encode_kernels_use_no_scratch_and_fit_two_per_cu(tmp_path):
    k = kernel_descriptors(tmp_path)
    found = {n: d for n, d in k.items() if "rs_wg_encode_list_kernel" in n}
    # one instantiation per 2t = 2, 4, 6, 8 (the first template argument)
    t2 = sorted(int(re.search(r"rs_wg_encode_list_kernelILi(\d+)E", n).group(1)) for n in found)
    assert t2 == [2, 4, 6, 8], sorted(found)
    for n, d in found.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0, (n, d)
    lds = _group_segments(tmp_path)
    for n in found:
        assert 0 < lds[n] <= 163840 // 2, (n, lds[n])  # at least two workgroups stay resident per CU
