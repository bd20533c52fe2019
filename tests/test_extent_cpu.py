"""CPU checks of the byte-extent calls (include/ppfs_ecc.h ppfs_ecc_*_extents_*): the ABI's symbols and the
entry's layout, argument checks that use no GPU, the extent kernels' code-object resources, and the
calls' host-side arithmetic (paritypartyfs_amd/csrc/extent_plan.hpp, tests/cpp/test_extent_plan.cpp)
under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")

EXTENT_SYMBOLS = ("ppfs_ecc_read_extents_device", "ppfs_ecc_write_extents_device", "ppfs_ecc_read_extents_host",
                  "ppfs_ecc_write_extents_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native
    return _native.lib()


def test_extent_symbols_are_part_of_the_abi(lib):
    from paritypartyfs_amd import _native
    assert set(EXTENT_SYMBOLS) <= set(_native.EXPORTED_SYMBOLS)
    for name in EXTENT_SYMBOLS:
        assert getattr(lib, name)  # exported by the library


def test_extent_dtype_is_the_c_struct():
    from paritypartyfs_amd import _native
    dt = _native.EXTENT_DTYPE
    assert dt.itemsize == 16
    assert [(n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names] == [
        ("pos", "<u8", 0), ("block", "<u4", 8), ("offset", "<u2", 12), ("length", "<u2", 14)]


def test_null_context_is_einval_without_gpu(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.ppfs_ecc_read_extents_device(None, p, 4, p, 2, p, 100, p, 1, None) == -22
    assert lib.ppfs_ecc_write_extents_device(None, p, 100, p, 4, p, 2, p, None) == -22
    assert lib.ppfs_ecc_read_extents_host(None, p, 4, p, 2, p, 100, p, 1) == -22
    assert lib.ppfs_ecc_write_extents_host(None, p, 100, p, 4, p, 2, p) == -22
    # ... also for an empty list
    assert lib.ppfs_ecc_read_extents_device(None, p, 4, p, 0, p, 100, p, 1, None) == -22
    assert lib.ppfs_ecc_write_extents_host(None, p, 100, p, 4, p, 0, p) == -22
    assert lib.ppfs_ecc_last_error()


def test_extent_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    copies = {n: d for n, d in k.items() if "extent_copy_kernel" in n}
    assert len(copies) == 2, sorted(k)  # both directions: pack and overlay
    index = {n: d for n, d in k.items() if "extent_index_kernel" in n}
    assert len(index) == 1, sorted(k)
    for n, d in {**copies, **index}.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)


def test_python_extent_calls_validate_their_buffers():
    """The EccEngine extent methods reject wrong dtypes, memory kinds and short buffers before the library
    sees them (checked on an object without a context: no GPU)."""
    import torch

    from paritypartyfs_amd import _native
    from paritypartyfs_amd.ecc import EccEngine

    eng = EccEngine.__new__(EccEngine)
    eng._h = ctypes.c_void_p()
    eng.raw_block_size, eng.data_size = 255, 249
    image = np.zeros(8 * 255, np.uint8)
    buf = np.zeros(100, np.uint8)
    ext = np.zeros(4, _native.EXTENT_DTYPE)
    for call in (lambda e, **kw: eng.read_extents_host(image, e, buf, **kw),
                 lambda e, **kw: eng.write_extents_host(buf, image, e, **kw)):
        with pytest.raises(ValueError):
            call(ext.view(np.uint8))  # extents dtype
        with pytest.raises(ValueError):
            call(np.zeros(8, _native.EXTENT_DTYPE)[::2])  # not contiguous
        with pytest.raises(ValueError):
            call(ext, status=np.zeros(3, np.uint8))  # short status
        with pytest.raises(ValueError):
            call(torch.zeros(64, dtype=torch.uint8))  # a tensor is no host buffer
    with pytest.raises(ValueError):
        eng.read_extents_host(image, ext, buf.astype(np.int8))  # buffer dtype
    with pytest.raises(ValueError):
        eng.read_extents_host(torch.zeros(8 * 255, dtype=torch.uint8), ext, buf)  # image kind
    with pytest.raises(ValueError):
        eng.write_extents_host(buf, None, ext)  # no image
    t_image = torch.zeros(8 * 255, dtype=torch.uint8)
    t_buf = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(ValueError):
        eng.read_extents(t_image, ext, t_buf)  # host tensors
    with pytest.raises(ValueError):
        eng.write_extents(t_buf, t_image, ext)
    with pytest.raises(ValueError):
        eng.read_extents(t_image, torch.zeros(64, dtype=torch.uint8), t_buf)  # extents on the host
    with pytest.raises(ValueError):
        eng.read_extents(image, ext, buf)  # numpy arrays are no device buffers
    eng._h = None  # nothing to destroy


def test_file_extents_walks_like_read_file():
    from paritypartyfs_amd.block_device import file_extents

    ds = 249
    blocks = [7, 3, 9, 4]
    e = file_extents(blocks, 100, 149 + 249 + 2, ds)
    assert [tuple(int(v) for v in x) for x in e] == [(0, 7, 100, 149), (149, 3, 0, 249), (398, 9, 0, 2)]
    e = file_extents(blocks[:1], 3, 5, ds)  # the single-block file: head = tail
    assert [tuple(int(v) for v in x) for x in e] == [(0, 7, 3, 5)]
    assert e.dtype.itemsize == 16
    for off0 in (0, 1, ds - 1):
        for tail in (1, ds - 1, ds):
            nbytes = (ds - off0) + ds + tail
            e = file_extents(blocks, off0, nbytes, ds)
            assert len(e) == 3 and int(e["length"].sum()) == nbytes
            assert list(e["pos"]) == [0, ds - off0, 2 * ds - off0] and list(e["offset"]) == [off0, 0, 0]
            assert int(e["length"][-1]) == tail
    assert len(file_extents(blocks, 0, 0, ds)) == 0 and len(file_extents(blocks, 0, 10, 0)) == 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("extent_plan") / "test_extent_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_extent_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_extent_plan(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
