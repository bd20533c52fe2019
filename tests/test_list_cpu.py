"""CPU checks of the block-list calls (include/ppfs_ecc.h ppfs_ecc_*_list_*): argument checks that use
no GPU, the gather / scatter kernels' code-object resources, and the calls' host-side arithmetic
(paritypartyfs_amd/csrc/list_plan.hpp, tests/cpp/test_list_plan.cpp) under the address and
undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")

LIST_SYMBOLS = ("ppfs_ecc_decode_list_device", "ppfs_ecc_encode_list_device", "ppfs_ecc_write_list_device",
                "ppfs_ecc_decode_list_host", "ppfs_ecc_encode_list_host", "ppfs_ecc_write_list_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native
    return _native.lib()


def test_list_symbols_are_part_of_the_abi():
    from paritypartyfs_amd import _native
    assert set(LIST_SYMBOLS) <= set(_native.EXPORTED_SYMBOLS)
    assert _native.STATUS_OUT_OF_BOUNDS == 9


def test_null_context_is_einval_without_gpu(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.ppfs_ecc_decode_list_device(None, p, 4, p, 2, p, p, 1, None, None) == -22
    assert lib.ppfs_ecc_encode_list_device(None, p, p, 4, p, 2, None) == -22
    assert lib.ppfs_ecc_write_list_device(None, p, p, 4, p, p, 2, None) == -22
    assert lib.ppfs_ecc_decode_list_host(None, p, 4, p, 2, p, p, 1, None) == -22
    assert lib.ppfs_ecc_encode_list_host(None, p, p, 4, p, 2) == -22
    assert lib.ppfs_ecc_write_list_host(None, p, p, 4, p, p, 2) == -22
    # ... also for an empty list
    assert lib.ppfs_ecc_decode_list_device(None, p, 4, p, 0, p, p, 1, None, None) == -22
    assert lib.ppfs_ecc_last_error()


def test_list_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in ("gather_blocks_kernel", "scatter_blocks_kernel"):
        found = {n: d for n, d in k.items() if frag in n}
        assert found, (frag, sorted(k))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0, (n, d)


def test_python_list_calls_validate_their_buffers():
    """The EccEngine list methods reject wrong dtypes, memory kinds and short buffers before the library
    sees them (checked on an object without a context: no GPU)."""
    import numpy as np
    import torch

    from paritypartyfs_amd.ecc import EccEngine

    eng = EccEngine.__new__(EccEngine)
    eng._h = ctypes.c_void_p()
    eng.raw_block_size, eng.data_size = 255, 249
    image = np.zeros(8 * 255, np.uint8)
    data = np.zeros(4 * 249, np.uint8)
    ix = np.arange(4, dtype=np.uint32)
    with pytest.raises(ValueError):
        eng.decode_list_host(image, ix.astype(np.int64), data)  # index dtype
    with pytest.raises(ValueError):
        eng.decode_list_host(image, ix, data[:-1])  # short payload buffer
    with pytest.raises(ValueError):
        eng.decode_list_host(image, ix, data, status=np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        eng.encode_list_host(data[:-1], image, ix)
    with pytest.raises(ValueError):
        eng.write_list_host(data, image, ix, status=np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        eng.decode_list_host(torch.zeros(8 * 255, dtype=torch.uint8), ix, data)  # a tensor is no host buffer
    t_image = torch.zeros(8 * 255, dtype=torch.uint8)
    t_ix = torch.arange(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.decode_list(t_image, t_ix)  # host tensors
    with pytest.raises(ValueError):
        eng.encode_list(torch.zeros(4 * 249, dtype=torch.uint8), t_image, t_ix)
    with pytest.raises(ValueError):
        eng.write_list(torch.zeros(4 * 249, dtype=torch.uint8), t_image, t_ix)
    eng._h = None  # nothing to destroy


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("list_plan") / "test_list_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_list_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_list_plan(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
