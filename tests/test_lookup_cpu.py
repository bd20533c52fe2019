"""CPU checks of the directory lookups (include/ppfs_ecc.h ppfs_ecc_lookup_*): the rule (csrc/lookup_plan.hpp,
tests/cpp/test_lookup_plan.cpp) under the address and undefined-behaviour sanitizers, the new ABI without a GPU, the
Python loop that defines IBlockDevice.lookup on a device without a codec, and the new kernels' code-object resources.
The calls themselves need a context, which cannot be made without a GPU: tests/test_gpu_lookup.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_kernel_resources import kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritypartyfs_amd", "_lib", "libppfs_ecc.so")
NAMES = ("ppfs_ecc_lookup_plan", "ppfs_ecc_lookup_device", "ppfs_ecc_lookup_host")
KERNELS = ("lookup_match_kernel", "lookup_finish_kernel")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lookup_plan") / "test_lookup_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_lookup_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def test_lookup_plan(plan_exe):
    """The matcher against a literal strlen / strncmp restatement of _findEntryByName over exact-size heap blocks
    (lengths 0, 1, 11, 12, 13, 123, prefixes both ways, garbage behind the NUL, duplicates, the unterminated entry and
    the over-long queries against the stated rule), and the failure rule against a literal batch loop over a fake
    readFile for ds in {1, 3, 127, 128, 129, 249, 4091} x n in {0, 1, 255, 256, 257, 300, 513} x every (match, failing
    block) pair; every outcome class is non-empty."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"pairs: (\d+) found, (\d+) not found, (\d+) failed before, (\d+) failed behind, (\d+) failed without a match, "
                  r"(\d+) failing behind", r.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), r.stdout[-500:]


def test_lookup_calls_are_part_of_the_abi():
    from paritypartyfs_amd import _native, ecc
    from paritypartyfs_amd.block_device import FsError, IBlockDevice
    from paritypartyfs_amd.ecc import EccEngine

    header = open(os.path.join(ROOT, "include", "ppfs_ecc.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\((const )?ppfs_ecc_ctx\* ctx,", header, flags=re.M), name
    for method in ("lookup_plan", "lookup", "lookup_host", "lookup_names"):
        assert callable(getattr(EccEngine, method))
    assert callable(IBlockDevice.lookup)
    assert ecc.LOOKUP_QUERY_DTYPE is _native.LOOKUP_QUERY_DTYPE and ecc.LOOKUP_HIT_DTYPE is _native.LOOKUP_HIT_DTYPE
    assert ecc.LookupCounts._fields[:4] == ("found", "not_found", "failed", "out_of_range")
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

    for struct, dtype, size in (("ppfs_ecc_lookup_query", _native.LOOKUP_QUERY_DTYPE, 8),
                                ("ppfs_ecc_lookup_hit", _native.LOOKUP_HIT_DTYPE, 16)):
        f = fields(struct)
        assert [n for n, _ in f] == list(dtype.names) and sum(b for _, b in f) == size == dtype.itemsize
        at = 0
        for n, b in f:
            assert dtype.fields[n][1] == at and dtype.fields[n][0].itemsize == b
            at += b
    counts = fields("ppfs_ecc_lookup_counts")
    assert sum(b for _, b in counts) == 64 == ctypes.sizeof(_native.LookupCounts) and len(ecc.LookupCounts._fields) == 8
    assert [n for n, _ in counts][:4] == [n for n, _ in _native.LookupCounts._fields_][:4]
    # the new status: one value in the header, the plan and the binding, and none of the other statuses
    status = re.search(r"^#define PPFS_ECC_NOT_FOUND (\d+)\b", header, flags=re.M)
    assert status and int(status.group(1)) == _native.STATUS_NOT_FOUND and _native.STATUS_NOT_FOUND not in (0, 1, 5, 9, 255)
    plan = open(os.path.join(ROOT, "paritypartyfs_amd", "csrc", "lookup_plan.hpp")).read()
    assert re.search(rf"ST_NOT_FOUND = {_native.STATUS_NOT_FOUND},", plan) and "DEVIATION" in plan
    # the reference's values (lib/common/include/ppfs/common/types.hpp)
    assert FsError.PpFS_NotFound == 19 and FsError.DirectoryManager_NotFound == 7


def test_lookup_calls_of_a_null_context_without_gpu():
    if not os.path.exists(LIB):
        pytest.skip("engine library not built (run __graft_entry__.build())")
    from paritypartyfs_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(256)
    dirs, q = np.zeros(1, _native.FILE_DTYPE), np.zeros(1, _native.LOOKUP_QUERY_DTYPE)
    slots, totals = np.zeros(1, _native.FILES_SLOT_DTYPE), np.zeros(1, _native.FILES_TOTALS_DTYPE)
    assert lib.ppfs_ecc_lookup_plan(None, dirs.ctypes.data, 1, slots.ctypes.data, totals.ctypes.data) == -22
    assert lib.ppfs_ecc_last_error()
    for nq in (1, 0):
        assert lib.ppfs_ecc_lookup_device(None, buf, 1, dirs.ctypes.data, 1, q.ctypes.data, buf, nq, 0, buf, 256, buf, None, buf,
                                          None, None, 1, None) == -22
        assert lib.ppfs_ecc_lookup_host(None, buf, 1, dirs.ctypes.data, 1, q.ctypes.data, buf, nq, 0, buf, 256, buf, None, buf,
                                        None, None, 1) == -22
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_lookup_loop_on_a_raw_device():
    """IBlockDevice.lookup, the defining loop, on a device without a codec: names, prefixes, the empty name, garbage
    behind a NUL, duplicates, an unterminated entry, over-long queries, the inode mode, both batches of a directory of
    300 entries and an empty directory."""
    from paritypartyfs_amd import _native
    from paritypartyfs_amd.block_device import FsError, HeapDisk, RawBlockDevice
    from paritypartyfs_amd.ecc import EccEngine

    bs = 96  # no entry is block-aligned
    names = [b"f%03d" % i for i in range(300)]
    names[7], names[9], names[270], names[280] = b"twice", b"twice", b"late", b""
    entries = np.full((300, 128), 0xEE, np.uint8)
    for i, nm in enumerate(names):
        entries[i, :4] = np.frombuffer(np.uint32(1000 + i).tobytes(), np.uint8)
        entries[i, 4:4 + len(nm)] = np.frombuffer(nm, np.uint8)
        entries[i, 4 + len(nm)] = 0
    entries[11, 4:] = np.frombuffer(b"u" * 124, np.uint8)  # unterminated
    nblocks = -(-entries.size // bs)
    assert nblocks <= 12 + bs // 4 + (bs // 4) ** 2
    disk = HeapDisk((nblocks + 40) * bs)
    dev = RawBlockDevice(bs, disk)
    # data blocks 0 .., index blocks behind them
    data = np.zeros(nblocks * bs, np.uint8)
    data[:entries.size] = entries.reshape(-1)
    disk.buf[:data.size] = data
    ipb, nxt = bs // 4, nblocks
    d = np.zeros(3, _native.FILE_DTYPE)
    d["direct"][0] = np.arange(12)
    ind = np.zeros(ipb, "<u4")
    ind[:] = 12 + np.arange(ipb)
    d["indirect"][0], nxt = nxt, nxt + 1
    disk.buf[int(d["indirect"][0]) * bs:][:4 * ipb] = ind.view(np.uint8)
    dbl = np.zeros(ipb, "<u4")
    d["doubly_indirect"][0], nxt = nxt, nxt + 1
    left, at = nblocks - 12 - ipb, 12 + ipb
    for k in range(-(-left // ipb)):
        leaf = np.zeros(ipb, "<u4")
        cnt = min(ipb, nblocks - at)
        leaf[:cnt] = at + np.arange(cnt)
        dbl[k], at = nxt, at + cnt
        disk.buf[nxt * bs:][:4 * ipb] = leaf.view(np.uint8)
        nxt += 1
    disk.buf[int(d["doubly_indirect"][0]) * bs:][:4 * ipb] = dbl.view(np.uint8)
    d["file_size"][0] = 300 * 128 + 77  # trailing bytes are never read
    d["direct"][1], d["file_size"][1] = np.arange(12), 5 * 128  # the first five entries as a directory of their own
    d["file_size"][2] = 100  # no entry

    ask = [(0, b"f000"), (0, b"f299"), (0, b"twice"), (0, b"late"), (0, b""), (0, b"f00"), (0, b"f0000"), (0, b"u" * 123),
           (0, b"nope"), (1, b"f004"), (1, b"f005"), (2, b"f000"), (0, b"twice")]
    q = np.zeros(len(ask) + 2, _native.LOOKUP_QUERY_DTYPE)
    q["dir"][:len(ask)] = [a for a, _ in ask]
    rec = np.zeros((len(ask) + 2, 128), np.uint8)
    rec[:len(ask)] = EccEngine.lookup_names([n for _, n in ask])
    rec[len(ask)] = np.frombuffer(b"u" * 128, np.uint8)  # no NUL
    rec[len(ask) + 1, :124] = np.frombuffer(b"u" * 124, np.uint8)  # L = 124
    got = dev.lookup(d, q, rec, 0)
    nf = (None, None, FsError.PpFS_NotFound)
    assert got == [(1000, 0, None), (1299, 299, None), (1007, 7, None), (1270, 270, None), (1280, 280, None), nf, nf, nf, nf,
                   (1004, 4, None), nf, nf, (1007, 7, None), nf, nf]
    qi = np.zeros(4, _native.LOOKUP_QUERY_DTYPE)
    qi["dir"], qi["key"] = [0, 0, 1, 2], [1299, 5, 1003, 1000]
    assert dev.lookup(d, qi, None, 1) == [(1299, 299, None), (None, None, FsError.DirectoryManager_NotFound), (1003, 3, None),
                                          (None, None, FsError.DirectoryManager_NotFound)]
    qi["dir"][1] = 3  # names no directory of the call
    assert dev.lookup(d, qi, None, 1)[1] == (None, None, FsError.DirectoryManager_InvalidRequest)
    with pytest.raises(ValueError):
        EccEngine.lookup_names([b"x" * 124])


def test_lookup_kernels_use_no_scratch(tmp_path):
    k = kernel_descriptors(tmp_path)
    for frag in KERNELS:
        found = {n: d for n, d in k.items() if frag in n}
        assert len(found) == 1, (frag, sorted(found))
        for n, d in found.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
