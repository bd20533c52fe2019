"""Python mirror of PPFS's block-device layer, backed by the MI355X ECC engine.

Same class names, constructor arguments, return conventions and error behaviour as the
reference (lib/blockdevice/include/ppfs/blockdevice/*.hpp, iblock_device.hpp:34-97), so the
parity tests read like the reference's unit tests:

  - ``writeBlock(data, DataLocation(i, off)) -> Expected[int]`` (bytes written)
  - ``readBlock(DataLocation(i, off), n, capacity=None) -> Expected[bytes]``
  - ``rawBlockSize() / dataSize() / numOfBlocks() / formatBlock(i)``

All codec arithmetic runs in the HIP kernels (EccEngine host path); this layer only moves
bytes between the disk and the engine and reproduces the reference's read-modify-write,
write-back and logging order.  Batched ``readBlocks`` / ``writeBlocks`` run a contiguous
range of blocks through one engine call (the GPU-worthwhile form);
``readBlockList`` / ``writeBlockList`` do so for blocks in any order, ``read_extents`` /
``write_extents`` for byte ranges (block, offset, length) of them -- a file range built by
``file_extents``, or a few bytes of an inode or bitmap block; ``file_blocks`` / ``read_file``
take the inode's 64-byte tree record (``FILE_DTYPE``) and resolve the index blocks themselves.
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass
from typing import Generic, List, Optional, Tuple, TypeVar

import numpy as np

from ._native import (ECC_CRC, ECC_HAMMING, ECC_NONE, ECC_PARITY, ECC_REED_SOLOMON, EXTENT_DTYPE, FILE_DTYPE, INODE_META_DTYPE, INODE_TABLE_DTYPE, LOOKUP_QUERY_DTYPE, STATUS_CORRECTED,
                      STATUS_CORRECTION_ERROR, STATUS_NOT_ALLOCATED, STATUS_NOT_FOUND, STATUS_OK, STATUS_OUT_OF_BOUNDS, EccError)
from .ecc import EccEngine, ScrubCounts

MAX_BLOCK_SIZE = 4096  # iblock_device.hpp:3
MAX_RS_BLOCK_SIZE = 255  # rs_block_device.hpp:7


class ECCType(enum.IntEnum):  # ecc_type.hpp:8-14
    None_ = ECC_NONE
    Crc = ECC_CRC
    Hamming = ECC_HAMMING
    Parity = ECC_PARITY
    ReedSolomon = ECC_REED_SOLOMON


class FsError(enum.IntEnum):  # lib/common/include/ppfs/common/types.hpp:11-80 (block-device subset)
    Bitmap_IndexOutOfRange = 0
    Bitmap_NotFound = 1
    BlockManager_AlreadyTaken = 2
    BlockManager_AlreadyFree = 3
    BlockManager_NoMoreFreeBlocks = 4
    BlockDevice_CorrectionError = 5
    DirectoryManager_NameTaken = 6
    DirectoryManager_NotFound = 7
    DirectoryManager_InvalidRequest = 8
    Disk_OutOfBounds = 9
    Disk_InvalidRequest = 10
    Disk_IOError = 11
    FileIO_OutOfBounds = 12
    PpFS_NotFound = 19
    InodeManager_NotFound = 26


# the packed Inode (inode.hpp:18-41), 81 bytes: what IBlockDevice.read_inodes delivers per inode
INODE_DTYPE = np.dtype([("time_creation", "<u8"), ("time_modified", "<u8"), ("direct", "<u4", (12,)), ("indirect", "<u4"),
                        ("doubly_indirect", "<u4"), ("trebly_indirect", "<u4"), ("file_size", "<u4"), ("type", "u1")])
assert INODE_DTYPE.itemsize == 81

T = TypeVar("T")


class Expected(Generic[T]):
    """std::expected<T, FsError> stand-in."""

    __slots__ = ("_v", "_e")

    def __init__(self, value: T = None, error: Optional[FsError] = None):
        self._v, self._e = value, error

    @staticmethod
    def unexpected(e: FsError) -> "Expected":
        return Expected(None, FsError(e))

    def has_value(self) -> bool:
        return self._e is None

    __bool__ = has_value

    def value(self) -> T:
        if self._e is not None:
            raise RuntimeError(f"bad expected access: {self._e.name}")
        return self._v

    def error(self) -> FsError:
        return self._e


@dataclass
class DataLocation:  # iblock_device.hpp:14-20
    block_index: int
    offset: int = 0


# ------------------------------------------------------------------------------------
# Disks (lib/disk): byte-addressed, out-of-range accesses fail whole (stack_disk.hpp:19-44)
# ------------------------------------------------------------------------------------
class IDisk:
    def read(self, address: int, size: int) -> Expected[bytes]:
        raise NotImplementedError

    def write(self, address: int, data) -> Expected[int]:
        raise NotImplementedError

    def size(self) -> int:
        raise NotImplementedError


class HeapDisk(IDisk):
    def __init__(self, size: int):
        self.buf = np.zeros(int(size), dtype=np.uint8)

    def size(self) -> int:
        return int(self.buf.size)

    def read(self, address: int, size: int) -> Expected[bytes]:
        if address + size > self.buf.size:
            return Expected.unexpected(FsError.Disk_OutOfBounds)
        return Expected(self.buf[address:address + size].tobytes())

    def write(self, address: int, data) -> Expected[int]:
        d = np.frombuffer(bytes(data), dtype=np.uint8)
        if address + d.size > self.buf.size:
            return Expected.unexpected(FsError.Disk_OutOfBounds)
        self.buf[address:address + d.size] = d
        return Expected(int(d.size))


class StackDisk(HeapDisk):
    """StackDisk<power> (default 2^22 bytes, zero-initialised)."""

    def __init__(self, power: int = 22):
        super().__init__(1 << power)


# ------------------------------------------------------------------------------------
# Logger (lib/data_collection): only ErrorCorrectionEvent is emitted by block devices
# ------------------------------------------------------------------------------------
class Logger:
    def __init__(self):
        self.corrections: List[Tuple[str, int]] = []

    def logEvent(self, kind: str, block_index: int) -> None:
        self.corrections.append((kind, int(block_index)))


# ------------------------------------------------------------------------------------
# CrcPolynomial (lib/ecc_helpers/src/crc_polynomial.cpp)
# ------------------------------------------------------------------------------------
class CrcPolynomial:
    def __init__(self, explicit_poly: int):
        self._p = int(explicit_poly)
        self._n = self._p.bit_length() - 1  # _findDegree :7-17

    @staticmethod
    def MsgExplicit(p: int) -> "CrcPolynomial":  # :27-39
        return CrcPolynomial(p)

    @staticmethod
    def MsgImplicit(p: int) -> "CrcPolynomial":  # :41-54
        return CrcPolynomial(((int(p) << 1) + 1) & 0xFFFFFFFFFFFFFFFF)

    def getDegree(self) -> int:
        return self._n

    def getExplicitPolynomial(self) -> int:
        return self._p

    def getCoefficients(self) -> List[bool]:  # MSB first, with the explicit +1
        return [bool((self._p >> (self._n - j)) & 1) for j in range(self._n + 1)]


# ------------------------------------------------------------------------------------
# Block devices
# ------------------------------------------------------------------------------------
class IBlockDevice:
    _engine: Optional[EccEngine] = None

    def rawBlockSize(self) -> int:
        raise NotImplementedError

    def dataSize(self) -> int:
        raise NotImplementedError

    def numOfBlocks(self) -> int:
        return self._disk.size() // self.rawBlockSize()

    # batch API: whole blocks [first, first+count); the per-block loop (codecs override it with
    # one engine call per range)
    def readBlocks(self, first: int, count: int) -> Tuple[np.ndarray, np.ndarray]:
        """Decode `count` whole blocks; returns (payloads [count, dataSize], FsError-or-0 per block)."""
        out = np.zeros((count, self.dataSize()), dtype=np.uint8)
        err = np.zeros(count, dtype=np.uint8)
        for i in range(count):
            r = self.readBlock(DataLocation(first + i, 0), self.dataSize())
            if r:
                out[i] = np.frombuffer(r.value(), dtype=np.uint8)
            else:
                err[i] = int(r.error())
        return out, err

    def scrub(self, first: int = 0, count: Optional[int] = None) -> Tuple[Tuple[int, int, int], np.ndarray]:
        """Whole-image scrub: the disk and log effect of readBlock(DataLocation(i, 0),
        dataSize()) for i in [first, first+count), in order, without the payloads.
        Returns ((ok, corrected, failed) block counts, FsError-or-0 per block)."""
        count = self.numOfBlocks() - first if count is None else count
        _, err = self.readBlocks(first, count)
        failed = int(np.count_nonzero(err))
        return (count - failed, 0, failed), err

    # scrub of named blocks only (include/ppfs_ecc.h ppfs_ecc_scrub_list_* / ppfs_ecc_scrub_allocated_*): the
    # per-block loops; the codecs override them with one engine call
    def bitmapBlocks(self, nbits: int) -> int:
        """Bitmap::blocksSpanned (bitmap.cpp:27-31) in integer arithmetic."""
        return -(-(-(-int(nbits) // 8)) // self.dataSize())

    def _log_count(self) -> int:
        logger = getattr(self, "_logger", None)
        return len(logger.corrections) if logger is not None else 0

    def scrubList(self, indices) -> Tuple[ScrubCounts, np.ndarray]:
        """The disk and log effect of readBlock(DataLocation(i, 0), dataSize()) for i in indices, in list
        order, without the payloads.  Returns (ScrubCounts, FsError-or-0 per entry)."""
        log0 = self._log_count()
        _, err = self.readBlockList(indices)
        corrected = self._log_count() - log0
        oob = int(np.count_nonzero(err == int(FsError.Disk_OutOfBounds)))
        failed = int(np.count_nonzero(err)) - oob
        return ScrubCounts(len(err) - failed - oob - corrected, corrected, failed, oob, 0, 0, 0, 0), err

    def scrubAllocated(self, bitmap_block: int, first_data_block: int, nbits: int) -> Tuple[ScrubCounts, np.ndarray, np.ndarray]:
        """Scrub of the blocks first_data_block + j whose bit j is set in the on-disk bitmap (lib/bitmap/src/
        bitmap.cpp) of nbits bits that starts at bitmap_block: the bitmap's own blocks are read first, then the
        allocated blocks in ascending order; all bits of a bitmap block that cannot be read count as set.
        Returns (ScrubCounts, per bit: 0 or the FsError, 255 where the bit is clear and the block was not
        read, FsError-or-0 per bitmap block)."""
        ds, B = self.dataSize(), self.bitmapBlocks(nbits)
        bitmap_err = np.zeros(B, dtype=np.uint8)
        bits = np.zeros(nbits, dtype=bool)
        bc = [0, 0, 0]
        for b in range(B):
            log0 = self._log_count()
            r = self.readBlock(DataLocation(bitmap_block + b, 0), ds)
            lo, hi = b * 8 * ds, min(nbits, (b + 1) * 8 * ds)
            if r:
                bits[lo:hi] = np.unpackbits(np.frombuffer(r.value(), dtype=np.uint8))[:hi - lo].astype(bool)
                bc[1 if self._log_count() > log0 else 0] += 1
            else:
                bitmap_err[b] = int(r.error())
                bits[lo:hi] = True
                bc[2] += 1
        alloc = np.nonzero(bits)[0]
        c, e = self.scrubList(first_data_block + alloc)
        err = np.full(nbits, STATUS_NOT_ALLOCATED, dtype=np.uint8)
        err[alloc] = e
        return ScrubCounts(c.ok, c.corrected, c.failed, c.out_of_range, nbits - alloc.size, *bc), err, bitmap_err

    def writeBlocks(self, first: int, payloads: np.ndarray) -> np.ndarray:
        err = np.zeros(len(payloads), dtype=np.uint8)
        for i, p in enumerate(payloads):
            r = self.writeBlock(bytes(p), DataLocation(first + i, 0))
            if not r:
                err[i] = int(r.error())
        return err


    # list API: whole blocks, any order -- what FileIO's BlockIndexIterator loop collects for a
    # fragmented file (file_io.cpp:27-35, 53-69).  The per-block loop; the codecs override it.
    def readBlockList(self, indices) -> Tuple[np.ndarray, np.ndarray]:
        """== readBlock(DataLocation(i, 0), dataSize()) for i in indices, in list order; returns
        (payloads [len(indices), dataSize], FsError-or-0 per entry)."""
        indices = [int(i) for i in indices]
        out = np.zeros((len(indices), self.dataSize()), dtype=np.uint8)
        err = np.zeros(len(indices), dtype=np.uint8)
        for k, i in enumerate(indices):
            r = self.readBlock(DataLocation(i, 0), self.dataSize())
            if r:
                out[k] = np.frombuffer(r.value(), dtype=np.uint8)
            else:
                err[k] = int(r.error())
        return out, err

    def writeBlockList(self, indices, payloads: np.ndarray) -> np.ndarray:
        """== writeBlock(payload_k, DataLocation(indices[k], 0)) in list order (full-block writes)."""
        indices = [int(i) for i in indices]
        payloads = np.ascontiguousarray(payloads, dtype=np.uint8).reshape(len(indices), -1)
        err = np.zeros(len(indices), dtype=np.uint8)
        for k, i in enumerate(indices):
            r = self.writeBlock(bytes(payloads[k]), DataLocation(i, 0))
            if not r:
                err[k] = int(r.error())
        return err


    # byte extents: entry k of `ext` (EXTENT_DTYPE: pos, block, offset, length) is one readBlock /
    # writeBlock at DataLocation(block, offset); its bytes lie at [pos, pos + len) of the packed buffer,
    # len = min(length, dataSize() - offset).  The per-block loop is the definition; the codecs
    # override it with one engine call.  An entry whose offset is past dataSize() or whose bytes do
    # not fit the buffer gets Disk_OutOfBounds and touches nothing.
    def _extent_len(self, e, buf_bytes: int) -> Optional[int]:
        """The clamped length of an entry; None when the entry is invalid before any block is read."""
        off, ds = int(e["offset"]), self.dataSize()
        if off > ds:
            return None
        n = min(int(e["length"]), ds - off)
        return n if int(e["pos"]) + n <= buf_bytes else None

    def read_extents(self, ext: np.ndarray, out: np.ndarray) -> np.ndarray:
        """== readBlock(DataLocation(block, offset), length) per entry, in list order, into
        out[pos, pos + len); returns FsError-or-0 per entry.  A failed entry's bytes become zeros; bytes
        of `out` that no entry covers keep their contents."""
        err = np.zeros(len(ext), dtype=np.uint8)
        for k, e in enumerate(ext):
            n = self._extent_len(e, out.size)
            if n is None:
                err[k] = int(FsError.Disk_OutOfBounds)
                continue
            pos = int(e["pos"])
            r = self.readBlock(DataLocation(int(e["block"]), int(e["offset"])), n)
            if r:
                out[pos:pos + n] = np.frombuffer(r.value(), dtype=np.uint8)
            else:
                err[k] = int(r.error())
                if err[k] != int(FsError.Disk_OutOfBounds):
                    out[pos:pos + n] = 0
        return err

    def write_extents(self, ext: np.ndarray, data: np.ndarray) -> np.ndarray:
        """== writeBlock(data[pos, pos + len), DataLocation(block, offset)) per entry, in list order."""
        err = np.zeros(len(ext), dtype=np.uint8)
        for k, e in enumerate(ext):
            n = self._extent_len(e, data.size)
            if n is None:
                err[k] = int(FsError.Disk_OutOfBounds)
                continue
            pos = int(e["pos"])
            r = self.writeBlock(data[pos:pos + n].tobytes(), DataLocation(int(e["block"]), int(e["offset"])))
            if not r:
                err[k] = int(r.error())
        return err

    # read a file from its inode (include/ppfs_ecc.h ppfs_ecc_file_blocks_* / ppfs_ecc_read_file_*): `file` is one
    # record of FILE_DTYPE.  The per-block loops are the definition -- the read-only BlockIndexIterator
    # (file_io.cpp:186-463) through readBlock: an index block is read, as readBlock({b, 0}, 4 ipb), immediately
    # before the first requested file block under it, outer levels first, each one once; the first error ends the
    # walk.  The codecs override both with engine calls on the whole tree.
    def _file_walk(self, file, first: int, count: int):
        """Yields the image block of file blocks first, first + 1, ... or, once and last, the FsError that ends the walk."""
        f = np.asarray(file).reshape(-1)[0]
        ds = self.dataSize()
        ipb = ds // 4
        occupied = -(-int(f["file_size"]) // ds) if ds else 0
        loaded = {}
        for j in range(first, first + count):
            p = file_path_of(j, ipb)
            if j >= occupied or p is None:
                yield FsError.FileIO_OutOfBounds
                return
            if p[0] == 0:
                yield int(f["direct"][j])
                continue
            pointer = int(f[("indirect", "doubly_indirect", "trebly_indirect")[p[0] - 1]])
            for d in range(1, len(p)):
                node = p[:d]
                if node not in loaded:
                    r = self.readBlock(DataLocation(pointer, 0), 4 * ipb)
                    if not r:
                        yield r.error()
                        return
                    loaded[node] = np.frombuffer(r.value(), dtype="<u4")
                pointer = int(loaded[node][p[d]])
            yield pointer

    def file_blocks(self, file, first: int, count: int) -> Tuple[np.ndarray, Optional[FsError]]:
        """The image blocks of file blocks [first, first + count): (those resolved before the first error, that
        error or None)."""
        out = []
        for v in self._file_walk(file, first, count):
            if isinstance(v, FsError):
                return np.array(out, dtype=np.uint32), v
            out.append(v)
        return np.array(out, dtype=np.uint32), None

    def read_file(self, file, offset: int, bytes_to_read: int) -> Tuple[bytes, Optional[FsError]]:
        """FileIO::readFile (file_io.cpp:12-44): (the bytes delivered before the first error, that error or None)."""
        f = np.asarray(file).reshape(-1)[0]
        size, ds = int(f["file_size"]), self.dataSize()
        if bytes_to_read <= 0:
            return b"", None
        if offset >= size or ds == 0:
            return b"", FsError.FileIO_OutOfBounds
        n = min(bytes_to_read, size - offset)
        first, count = offset // ds, (offset % ds + n + ds - 1) // ds
        out = bytearray()
        for k, v in enumerate(self._file_walk(file, first, count)):
            if isinstance(v, FsError):
                return bytes(out), v
            off = offset % ds if k == 0 else 0
            r = self.readBlock(DataLocation(v, off), min(ds - off, n - len(out)))
            if not r:
                return bytes(out), r.error()
            out += r.value()
        return bytes(out), None

    def read_files(self, files, ranges) -> List[Tuple[bytes, Optional[FsError]]]:
        """A batch of (inode, offset, length): == read_file(files[f], *ranges[f]) per file, in batch order (a directory
        scan, a backup).  The codecs override it with one engine walk over all the files' trees."""
        files = np.asarray(files).reshape(-1)
        return [self.read_file(files[f:f + 1], int(off), int(n)) for f, (off, n) in enumerate(ranges)]

    # write a file range from its inode (include/ppfs_ecc.h ppfs_ecc_write_file_* / ppfs_ecc_write_files_*): the in-place
    # case of FileIO::writeFile (file_io.cpp:46-104).  The range must lie inside the file; nothing is allocated and no
    # inode is updated.  The per-block loop is the definition: the walk above, one writeBlock per data block, the first
    # error ends it.  The codecs override both with one engine call.
    def write_file(self, file, offset: int, data) -> Tuple[int, Optional[FsError]]:
        """(the bytes written before the first error, that error or None)."""
        f = np.asarray(file).reshape(-1)[0]
        data = bytes(data)
        size, ds, n = int(f["file_size"]), self.dataSize(), len(data)
        if n == 0:
            return 0, None
        if ds == 0 or offset < 0 or offset + n > size:
            return 0, FsError.FileIO_OutOfBounds
        first, count = offset // ds, (offset % ds + n + ds - 1) // ds
        written = 0
        for k, v in enumerate(self._file_walk(file, first, count)):
            if isinstance(v, FsError):
                return written, v
            off = offset % ds if k == 0 else 0
            ln = min(ds - off, n - written)
            r = self.writeBlock(data[written:written + ln], DataLocation(v, off))
            if not r:
                return written, r.error()
            written += ln
        return written, None

    def write_files(self, files, ranges, datas) -> List[Tuple[int, Optional[FsError]]]:
        """A batch of (inode, offset, bytes): == write_file(files[f], ranges[f][0], datas[f][:ranges[f][1]]) per file, in
        batch order."""
        files = np.asarray(files).reshape(-1)
        return [self.write_file(files[f:f + 1], int(off), bytes(datas[f])[:max(int(n), 0)]) for f, (off, n) in enumerate(ranges)]

    # read inodes from the inode table (include/ppfs_ecc.h ppfs_ecc_read_inodes_*): `table` is one record of
    # INODE_TABLE_DTYPE, `numbers` the inode numbers.  The per-inode loop is the definition -- InodeManager::get
    # (inode_manager.cpp:127-138): Bitmap::getBit (bitmap.cpp:8-25, 87-101), a one-byte readBlock, then _readInode
    # (:56-89), the 81 bytes cut at block boundaries by a clamping readBlock; the first error ends that inode.  The
    # codecs override it with one engine call.
    def _inode_get_bit(self, bitmap_block: int, total: int, bit_index: int) -> Expected[bool]:
        if bit_index >= total:
            return Expected.unexpected(FsError.Bitmap_IndexOutOfRange)
        ds = self.dataSize()
        byte = bit_index // 8
        r = self.readBlock(DataLocation(bitmap_block + byte // ds, byte % ds), 1)
        if not r:
            return Expected.unexpected(r.error())
        return Expected(((r.value()[0] >> (7 - bit_index % 8)) & 1) > 0)

    def _inode_read(self, table_block: int, index: int) -> Expected[bytes]:
        size, ds = INODE_DTYPE.itemsize, self.dataSize()
        inode = bytearray()
        start = DataLocation(table_block + index * size // ds, index * size % ds)
        if ds - start.offset < size:  # does not fit in one block: the unaligned part first
            r = self.readBlock(start, size)
            if not r:
                return Expected.unexpected(r.error())
            start = DataLocation(start.block_index + 1, 0)
            inode += r.value()
        while len(inode) < size:
            r = self.readBlock(start, size - len(inode))
            if not r:
                return Expected.unexpected(r.error())
            inode += r.value()
            start = DataLocation(start.block_index + 1, start.offset)
        return Expected(bytes(inode))

    def read_inodes(self, table, numbers) -> List[Tuple[Optional[np.void], Optional[FsError]]]:
        """InodeManager::get per inode number, in batch order: (the INODE_DTYPE record, None) or (None, the error).
        A set bit of the inode bitmap means free: InodeManager_NotFound.  table["check_bitmap"] == 0 skips the bit's
        read, not the range check."""
        t = np.asarray(table).reshape(-1)[0]
        table_block, bitmap_block, total = int(t["table_block"]), int(t["bitmap_block"]), int(t["total_inodes"])
        if self.dataSize() == 0:
            raise ValueError("read_inodes: the codec has no payload")
        out = []
        for i in (int(x) for x in np.asarray(numbers).reshape(-1)):
            if int(t["check_bitmap"]):
                free = self._inode_get_bit(bitmap_block, total, i)
                if not free:
                    out.append((None, free.error()))
                    continue
                if free.value():
                    out.append((None, FsError.InodeManager_NotFound))
                    continue
            elif i >= total:
                out.append((None, FsError.Bitmap_IndexOutOfRange))
                continue
            r = self._inode_read(table_block, i)
            out.append((np.frombuffer(r.value(), dtype=INODE_DTYPE)[0], None) if r else (None, r.error()))
        return out

    # write inodes into the inode table (include/ppfs_ecc.h ppfs_ecc_write_inodes_*): the arguments of read_inodes, and
    # per inode its FILE_DTYPE record and its INODE_META_DTYPE record.  The per-inode loop is the definition --
    # InodeManager::update (inode_manager.cpp:142-159): Bitmap::getBit, then _writeInode (:20-54), the 81 bytes cut at
    # block boundaries by a clamping writeBlock; the first error ends that inode.  The codecs override it with one
    # engine call.
    @staticmethod
    def _inode_pack(files, meta, n: int) -> np.ndarray:
        """The n packed Inodes (INODE_DTYPE) of the file records and the metadata; the metadata's padding is not used."""
        files = np.ascontiguousarray(files).reshape(-1).view(FILE_DTYPE)
        meta = np.ascontiguousarray(meta).reshape(-1).view(INODE_META_DTYPE)
        if files.size < n or meta.size < n:
            raise ValueError("write_inodes: one file record and one metadata record per inode number")
        rec = np.zeros(n, dtype=INODE_DTYPE)
        rec["time_creation"], rec["time_modified"], rec["type"] = meta["time_creation"][:n], meta["time_modified"][:n], meta["type"][:n]
        for name in FILE_DTYPE.names:
            rec[name] = files[name][:n]
        return rec

    def _inode_write(self, table_block: int, index: int, inode: bytes) -> Expected[None]:
        size, ds = INODE_DTYPE.itemsize, self.dataSize()
        written = 0
        start = DataLocation(table_block + index * size // ds, index * size % ds)
        if ds - start.offset < size:  # does not fit in one block: the unaligned part first
            r = self.writeBlock(inode, start)
            if not r:
                return Expected.unexpected(r.error())
            written += r.value()
            start = DataLocation(start.block_index + 1, 0)
        while written < size:
            r = self.writeBlock(inode[written:], start)
            if not r:
                return Expected.unexpected(r.error())
            written += r.value()
            start = DataLocation(start.block_index + 1, start.offset)
        return Expected(None)

    def write_inodes(self, table, numbers, files, meta) -> List[Optional[FsError]]:
        """InodeManager::update per inode number, in batch order: None or the error.  A set bit of the inode bitmap
        means free: InodeManager_NotFound, nothing written.  table["check_bitmap"] == 0 skips the bit's read, not the
        range check."""
        t = np.asarray(table).reshape(-1)[0]
        table_block, bitmap_block, total = int(t["table_block"]), int(t["bitmap_block"]), int(t["total_inodes"])
        if self.dataSize() == 0:
            raise ValueError("write_inodes: the codec has no payload")
        nums = [int(x) for x in np.asarray(numbers).reshape(-1)]
        rec = self._inode_pack(files, meta, len(nums))
        out = []
        for j, i in enumerate(nums):
            if int(t["check_bitmap"]):
                free = self._inode_get_bit(bitmap_block, total, i)
                if not free:
                    out.append(free.error())
                    continue
                if free.value():
                    out.append(FsError.InodeManager_NotFound)
                    continue
            elif i >= total:
                out.append(FsError.Bitmap_IndexOutOfRange)
                continue
            r = self._inode_write(table_block, i, rec[j].tobytes())
            out.append(None if r else r.error())
        return out

    # look up names in directories (include/ppfs_ecc.h ppfs_ecc_lookup_*): `dirs` is an array of FILE_DTYPE records,
    # `queries` one of LOOKUP_QUERY_DTYPE (dir: a number into dirs), `names` the queries' 128-byte name records (an
    # (n, 128) uint8 array; unused in inode mode).  The loop is the definition -- DirectoryManager::getInodeByName
    # (directory_manager.cpp:135-163) for mode 0, removeEntry's search (:67-90) up to and including the found_entry
    # decision for mode 1, both over _readDirectoryData (:165-187), a readFile of at most 256 entries.  DEVIATION: an
    # entry whose 124 name bytes hold no NUL matches nothing (the reference's strlen would run on).  The codecs override
    # it with one engine call.
    DIR_ENTRY_BYTES, DIR_ENTRY_BATCH = 128, 256

    @staticmethod
    def _c_string(b: bytes, cap: int) -> Optional[bytes]:
        """The bytes before the first NUL among the first cap bytes; None when there is no NUL."""
        at = bytes(b[:cap]).find(b"\0")
        return None if at < 0 else bytes(b[:at])

    def _read_directory_data(self, dir_inode, offset: int, size: int):  # :165-187
        max_entries = int(dir_inode["file_size"][0]) // self.DIR_ENTRY_BYTES
        if offset >= max_entries:
            return [], None
        size = min(size, max_entries - offset)
        data, err = self.read_file(dir_inode, offset * self.DIR_ENTRY_BYTES, size * self.DIR_ENTRY_BYTES)
        if err is not None:
            return None, err
        E = self.DIR_ENTRY_BYTES
        return [data[E * i:E * i + E] for i in range(len(data) // E)], None

    def lookup(self, dirs, queries, names=None, mode: int = 0) -> List[Tuple[Optional[int], Optional[int], Optional[FsError]]]:
        """Per query (inode, entry, None), or (None, None, error): the failing block's FsError, PpFS_NotFound (mode 0)
        or DirectoryManager_NotFound (mode 1); DirectoryManager_InvalidRequest for a `dir` at or past the directories."""
        dirs = np.asarray(dirs).reshape(-1)
        out = []
        for q, query in enumerate(np.asarray(queries).reshape(-1)):
            if int(query["dir"]) >= dirs.size:  # names no directory of the call
                out.append((None, None, FsError.DirectoryManager_InvalidRequest))
                continue
            dir_inode, key = dirs[int(query["dir"]):int(query["dir"]) + 1], int(query["key"])
            name = None
            if mode == 0:
                name = self._c_string(bytes(np.asarray(names[q], dtype=np.uint8).tobytes()), 128)
                if name is not None and len(name) >= 124:
                    name = None  # matches nothing
            num_entries = int(dir_inode["file_size"][0]) // self.DIR_ENTRY_BYTES
            checked, found, error = 0, None, None
            while checked < num_entries:
                entries, error = self._read_directory_data(dir_inode, checked, self.DIR_ENTRY_BATCH)
                if error is not None:
                    break
                for i, e in enumerate(entries):  # _findEntryByName (:189-199) / _findEntryByInode (:201-210)
                    inode = int.from_bytes(e[:4], "little")
                    if (mode == 0 and name is not None and self._c_string(e[4:], 124) == name) or (mode != 0 and inode == key):
                        found = (inode, checked + i)
                        break
                if found is not None:
                    break
                checked += len(entries)
            if error is not None:
                out.append((None, None, error))
            elif found is None:
                out.append((None, None, FsError.PpFS_NotFound if mode == 0 else FsError.DirectoryManager_NotFound))
            else:
                out.append((found[0], found[1], None))
        return out



def file_path_of(j: int, ipb: int):
    """Where file block j lies in an inode's tree (inode.hpp:18-41): (segment, slot at each index block from the
    root down), segment 0 = direct[j]; None past the tree's 12 + ipb + ipb^2 + ipb^3 blocks."""
    if j < 12:
        return (0, j)
    s = j - 12
    if s < ipb:
        return (1, s)
    s -= ipb
    if s < ipb * ipb:
        return (2, s // ipb, s % ipb)
    s -= ipb * ipb
    if s < ipb ** 3:
        return (3, s // (ipb * ipb), (s // ipb) % ipb, s % ipb)
    return None


def file_extents(indices, offset_in_first_block: int, nbytes: int, data_size: int) -> np.ndarray:
    """The entries of a FileIO::readFile / writeFile walk (file_io.cpp:24-42, 50-88) over the blocks
    `indices` (from the block that holds the first byte on): the first block from
    offset_in_first_block = offset % dataSize(), whole blocks after it, the last one up to where the
    nbytes run out; pos is the running sum, so the packed buffer is the file range itself."""
    out = []
    done = 0
    if data_size > 0 and 0 <= offset_in_first_block < data_size:
        for k, i in enumerate(indices):
            if done >= nbytes:
                break
            off = offset_in_first_block if k == 0 else 0
            n = min(data_size - off, nbytes - done)
            out.append((done, int(i), off, n))
            done += n
    return np.array(out, dtype=EXTENT_DTYPE)


def _list_runs(indices: List[int]):
    """[start, end) of the maximal stretches of a list in which no index repeats."""
    start, seen = 0, set()
    for k, i in enumerate(indices):
        if i in seen:
            yield start, k
            start, seen = k, set()
        seen.add(i)
    if start < len(indices):
        yield start, len(indices)


class RawBlockDevice(IBlockDevice):  # raw_block_device.cpp
    def __init__(self, block_size: int, disk: IDisk):
        self._bs, self._disk = int(block_size), disk

    def rawBlockSize(self) -> int:
        return self._bs

    def dataSize(self) -> int:
        return self._bs

    def formatBlock(self, block_index: int) -> Expected[None]:
        return Expected(None)

    def writeBlock(self, data, loc: DataLocation) -> Expected[int]:
        data = bytes(data)
        to_write = min(len(data), self._bs - loc.offset)
        r = self._disk.write(loc.block_index * self._bs + loc.offset, data[:to_write])
        return Expected(to_write) if r else Expected.unexpected(r.error())

    def readBlock(self, loc: DataLocation, bytes_to_read: int, capacity: Optional[int] = None) -> Expected[bytes]:
        to_read = min(bytes_to_read, self._bs - loc.offset)
        addr = loc.block_index * self._bs + loc.offset
        if addr + to_read > self._disk.size():
            return Expected.unexpected(FsError.Disk_OutOfBounds)
        if capacity is not None and capacity < to_read:
            return Expected.unexpected(FsError.Disk_InvalidRequest)
        return self._disk.read(addr, to_read)


class _EngineDevice(IBlockDevice):
    """Shared read-modify-write plumbing for the ECC codecs."""

    _log_name = ""

    def __init__(self, engine: EccEngine, disk: IDisk, logger: Optional[Logger]):
        self._engine, self._disk, self._logger = engine, disk, logger
        self._raw, self._ds = engine.raw_block_size, engine.data_size

    def rawBlockSize(self) -> int:
        return self._raw

    def dataSize(self) -> int:
        return self._ds

    def _read_raw(self, block_index: int) -> Expected[np.ndarray]:
        r = self._disk.read(block_index * self._raw, self._raw)
        if not r:
            return Expected.unexpected(r.error())
        return Expected(np.frombuffer(r.value(), dtype=np.uint8).copy())

    def _log(self, block_index: int) -> None:
        if self._logger is not None and self._log_name:
            self._logger.logEvent(self._log_name, block_index)

    # decode one old block on the GPU; apply the reference's write-back; returns payload
    def _check_fix(self, block_index: int, raw: np.ndarray) -> Expected[np.ndarray]:
        raise NotImplementedError

    def formatBlock(self, block_index: int) -> Expected[None]:
        r = self._disk.write(block_index * self._raw, bytes(self._raw))
        return Expected(None) if r else Expected.unexpected(r.error())

    # ---- batched whole-block I/O: one engine call per contiguous range ----
    def _has_spill(self) -> bool:
        return self._engine.ecc_type == ECC_REED_SOLOMON and self._raw < 255

    def _write_back(self, block_index: int, old: np.ndarray, fixed: np.ndarray, spill) -> Optional[FsError]:
        raise NotImplementedError

    def readBlocks(self, first: int, count: int) -> Tuple[np.ndarray, np.ndarray]:
        """== readBlock(DataLocation(i, 0), dataSize()) for i in [first, first+count), in order:
        same payloads, per-block errors, disk contents and correction log."""
        out = np.zeros((count, self._ds), dtype=np.uint8)
        err = np.zeros(count, dtype=np.uint8)
        e = self._engine
        wb = e.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        done = 0
        while done < count:
            nb = count - done
            r = self._disk.read((first + done) * self._raw, nb * self._raw)
            if not r:
                # range not on the disk: per-block calls report it block by block
                for i in range(done, count):
                    rr = self.readBlock(DataLocation(first + i, 0), self._ds)
                    if rr:
                        out[i] = np.frombuffer(rr.value(), dtype=np.uint8)
                    else:
                        err[i] = int(rr.error())
                break
            raw = np.frombuffer(r.value(), dtype=np.uint8).copy()
            fixed = raw.copy()
            status = np.zeros(nb, dtype=np.uint8)
            spill = np.zeros(nb * e.spill_bytes_per_block(), dtype=np.uint8) if self._has_spill() else None
            e.decode_host(fixed, out[done:].reshape(-1), status, write_back=wb, spill=spill)
            if spill is None:
                # no write-back leaves its block: the per-block write-backs together are the
                # changed bytes of the range, written once; the log keeps block order
                bad = np.nonzero(status == STATUS_CORRECTION_ERROR)[0]
                err[done + bad] = int(FsError.BlockDevice_CorrectionError)
                out[done + bad] = 0
                if wb:
                    for i in np.nonzero(status == STATUS_CORRECTED)[0]:
                        self._log(first + done + int(i))
                    changed = np.nonzero(fixed != raw)[0]
                    if changed.size:
                        lo, hi = int(changed[0]), int(changed[-1]) + 1
                        self._disk.write((first + done) * self._raw + lo, fixed[lo:hi].tobytes())
                done += nb
                continue
            i = 0
            while i < nb:
                st = int(status[i])
                if st == STATUS_CORRECTION_ERROR:
                    err[done + i] = int(FsError.BlockDevice_CorrectionError)
                    out[done + i] = 0
                elif st == STATUS_CORRECTED and wb:
                    sp = spill[i * e.spill_bytes_per_block():(i + 1) * e.spill_bytes_per_block()] \
                        if spill is not None else None
                    fe = self._write_back(first + done + i, raw[i * self._raw:(i + 1) * self._raw],
                                          fixed[i * self._raw:(i + 1) * self._raw], sp)
                    if fe is not None:
                        err[done + i] = int(fe)
                    if sp is not None and int(sp[0]) and i + 1 < nb:
                        i += 1  # the write-back ran into the next block: re-read from there
                        break
                i += 1
            done += i
        return out, err

    def scrub(self, first: int = 0, count: Optional[int] = None) -> Tuple[Tuple[int, int, int], np.ndarray]:
        """Whole-image scrub in one engine call (EccEngine.scrub_host): the disk
        image from block `first` to the disk end goes through ppfs_ecc_scrub_host, which applies
        the reference's read-path write-back block by block in index order (RS codeword incl.
        bytes past a shortened block, Hamming flipped byte); corrected blocks are logged in order.
        Returns ((ok, corrected, failed) block counts, FsError-or-0 per block)."""
        n_all = self.numOfBlocks()
        count = n_all - first if count is None else count
        base = first * self._raw
        r = self._disk.read(base, self._disk.size() - base) if 0 <= first and first + count <= n_all else None
        if not r:
            log0 = self._log_count()
            _, err = self.readBlocks(first, count)  # blocks off the disk: per-block semantics
            failed = int(np.count_nonzero(err))
            corrected = self._log_count() - log0
            return (count - failed - corrected, corrected, failed), err
        image = np.frombuffer(r.value(), dtype=np.uint8).copy()
        before = image.copy()
        status = np.zeros(count, dtype=np.uint8)
        counts = self._engine.scrub_host(image, nblocks=count, status=status)
        err = np.where(status == STATUS_CORRECTION_ERROR, int(FsError.BlockDevice_CorrectionError), 0).astype(np.uint8)
        for i in np.nonzero(status == STATUS_CORRECTED)[0]:
            self._log(first + int(i))
        changed = np.nonzero(image != before)[0]
        if changed.size:
            lo, hi = int(changed[0]), int(changed[-1]) + 1
            w = self._disk.write(base + lo, image[lo:hi].tobytes())
            if not w:
                err[:] = int(w.error())
        return counts, err

    def _scrub_image(self):
        """The whole disk image for one engine call on it, or None where the per-block loop has to run: a
        shortened RS code, whose write-back may run into the next block, and a disk that cannot be read whole."""
        if self._has_spill() or not self._raw or not self._ds:
            return None
        r = self._disk.read(0, self._disk.size())
        return np.frombuffer(r.value(), dtype=np.uint8).copy() if r else None

    def _scrub_done(self, image: np.ndarray, before: np.ndarray, status: np.ndarray, blocks) -> np.ndarray:
        """After an engine scrub of `image`: a correction event per status 1 in the order of `blocks`, the
        changed bytes onto the disk; returns the statuses as FsError-or-0 (5, 9 and 255 are kept)."""
        for k in np.nonzero(status == STATUS_CORRECTED)[0]:
            self._log(int(blocks[int(k)]))
        changed = np.nonzero(image != before)[0]
        if changed.size:
            lo, hi = int(changed[0]), int(changed[-1]) + 1
            self._disk.write(lo, image[lo:hi].tobytes())
        return np.where(status == STATUS_CORRECTED, 0, status).astype(np.uint8)

    def scrubList(self, indices) -> Tuple[ScrubCounts, np.ndarray]:
        """IBlockDevice.scrubList in one engine call (EccEngine.scrub_list_host) on the disk image."""
        image = self._scrub_image()
        if image is None:
            return super().scrubList(indices)
        ix = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        before, status = image.copy(), np.zeros(ix.size, dtype=np.uint8)
        counts = self._engine.scrub_list_host(image, ix, status=status)
        return counts, self._scrub_done(image, before, status, ix)

    def scrubAllocated(self, bitmap_block: int, first_data_block: int, nbits: int) -> Tuple[ScrubCounts, np.ndarray, np.ndarray]:
        """IBlockDevice.scrubAllocated in one engine call (EccEngine.scrub_allocated_host) on the disk image;
        the bitmap blocks' corrections are logged first, then the data blocks', each in ascending order."""
        image = self._scrub_image()
        B = self.bitmapBlocks(nbits) if self._ds else 0
        if image is None or bitmap_block + B > self.numOfBlocks():
            return super().scrubAllocated(bitmap_block, first_data_block, nbits)
        before, status, bst = image.copy(), np.zeros(nbits, dtype=np.uint8), np.zeros(B, dtype=np.uint8)
        counts = self._engine.scrub_allocated_host(image, bitmap_block, first_data_block, nbits, status=status,
                                                   bitmap_status=bst)
        blocks = np.concatenate([bitmap_block + np.arange(B), first_data_block + np.arange(nbits)])
        err = self._scrub_done(image, before, np.concatenate([bst, status]), blocks)
        return counts, err[B:], err[:B]

    def _log_count(self) -> int:
        return len(self._logger.corrections) if self._logger is not None else 0

    def writeBlocks(self, first: int, payloads: np.ndarray) -> np.ndarray:
        """== writeBlock(payload_i, DataLocation(first+i, 0)) in order (full-block writes)."""
        payloads = np.ascontiguousarray(payloads, dtype=np.uint8).reshape(-1, self._ds)
        count = payloads.shape[0]
        err = np.zeros(count, dtype=np.uint8)
        r = self._disk.read(first * self._raw, count * self._raw)
        if self._has_spill() or not r:
            return super().writeBlocks(first, payloads)  # per-block order (spill / out of range)
        raw = np.frombuffer(r.value(), dtype=np.uint8).copy()
        status = np.zeros(count, dtype=np.uint8)
        self._engine.write_host(payloads.reshape(-1), raw, status)
        for i in range(count):
            if status[i] == STATUS_CORRECTION_ERROR:
                err[i] = int(FsError.BlockDevice_CorrectionError)  # block left untouched
            elif status[i] == STATUS_CORRECTED:
                self._log(first + i)  # the old block's write-back is overwritten below
        w = self._disk.write(first * self._raw, raw.tobytes())
        if not w:
            err[:] = int(w.error())
        return err

    # ---- block lists: one engine call per stretch of the list without a repeated index ----
    def _on_disk(self, block_index: int) -> bool:
        return 0 <= block_index and (block_index + 1) * self._raw <= self._disk.size()

    def _list_rows(self, indices: List[int]):
        """(list positions of the entries that lie on the disk, their rows packed); None for the
        rows when a disk read failed (the caller then goes block by block)."""
        pos = [k for k, i in enumerate(indices) if self._on_disk(i)]
        rows = np.zeros(len(pos) * self._raw, dtype=np.uint8)
        for j, k in enumerate(pos):
            r = self._disk.read(indices[k] * self._raw, self._raw)
            if not r:
                return pos, None
            rows[j * self._raw:(j + 1) * self._raw] = np.frombuffer(r.value(), dtype=np.uint8)
        return pos, rows

    def readBlockList(self, indices) -> Tuple[np.ndarray, np.ndarray]:
        """== readBlock(DataLocation(i, 0), dataSize()) for i in indices, in list order: same
        payloads, per-entry errors, disk contents and correction log.  A block listed again is read
        as its earlier entry's write-back left it."""
        indices = [int(i) for i in indices]
        if self._has_spill():
            return super().readBlockList(indices)  # a write-back may run into the next block
        out = np.zeros((len(indices), self._ds), dtype=np.uint8)
        err = np.zeros(len(indices), dtype=np.uint8)
        e = self._engine
        wb = e.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        for s, t in _list_runs(indices):
            run = indices[s:t]
            pos, raw = self._list_rows(run)
            if raw is None:
                out[s:t], err[s:t] = super().readBlockList(run)
                continue
            for k in set(range(len(run))) - set(pos):  # off the disk: the per-block call's error
                r = self.readBlock(DataLocation(run[k], 0), self._ds)
                err[s + k] = int(r.error()) if not r else 0
            if not pos:
                continue
            fixed = raw.copy()
            status = np.zeros(len(pos), dtype=np.uint8)
            data = np.zeros(len(pos) * self._ds, dtype=np.uint8)
            e.decode_host(fixed, data, status, write_back=wb)
            data = data.reshape(len(pos), self._ds)
            for j, k in enumerate(pos):
                st = int(status[j])
                if st == STATUS_CORRECTION_ERROR:
                    err[s + k] = int(FsError.BlockDevice_CorrectionError)
                    continue
                out[s + k] = data[j]
                if st == STATUS_CORRECTED and wb:
                    fe = self._write_back(run[k], raw[j * self._raw:(j + 1) * self._raw],
                                          fixed[j * self._raw:(j + 1) * self._raw], None)
                    if fe is not None:
                        err[s + k] = int(fe)
        return out, err

    def writeBlockList(self, indices, payloads: np.ndarray) -> np.ndarray:
        """== writeBlock(payload_k, DataLocation(indices[k], 0)) in list order (full-block writes)."""
        indices = [int(i) for i in indices]
        payloads = np.ascontiguousarray(payloads, dtype=np.uint8).reshape(len(indices), self._ds)
        if self._has_spill():
            return super().writeBlockList(indices, payloads)
        err = np.zeros(len(indices), dtype=np.uint8)
        for s, t in _list_runs(indices):
            run = indices[s:t]
            pos, raw = self._list_rows(run)
            if raw is None:
                err[s:t] = super().writeBlockList(run, payloads[s:t])
                continue
            for k in set(range(len(run))) - set(pos):
                r = self.writeBlock(bytes(payloads[s + k]), DataLocation(run[k], 0))
                err[s + k] = int(r.error()) if not r else 0
            if not pos:
                continue
            status = np.zeros(len(pos), dtype=np.uint8)
            self._engine.write_host(np.ascontiguousarray(payloads[s:t][pos]).reshape(-1), raw, status)
            for j, k in enumerate(pos):
                if status[j] == STATUS_CORRECTION_ERROR:
                    err[s + k] = int(FsError.BlockDevice_CorrectionError)  # block left untouched
                    continue
                if status[j] == STATUS_CORRECTED:
                    self._log(run[k])  # the old block's write-back is overwritten below
                w = self._disk.write(run[k] * self._raw, raw[j * self._raw:(j + 1) * self._raw].tobytes())
                if not w:
                    err[s + k] = int(w.error())
        return err

    # ---- byte extents: one engine call on the disk's image, where the disk is one array in memory ----
    def _mapped_image(self) -> Optional[np.ndarray]:
        """The disk as the engine's host calls take it (a HeapDisk's array), unless a write-back may
        run into the next block (a shortened RS code): then the per-block loop stays."""
        buf = getattr(self._disk, "buf", None)
        if self._has_spill() or not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or not buf.flags["C_CONTIGUOUS"]:
            return None
        return buf

    def _extent_errors(self, ext: np.ndarray, status: np.ndarray) -> np.ndarray:
        """FsError-or-0 per entry from the engine's statuses; a correction event per status 1, in list order."""
        err = np.zeros(len(ext), dtype=np.uint8)
        err[status == STATUS_CORRECTION_ERROR] = int(FsError.BlockDevice_CorrectionError)
        err[status == STATUS_OUT_OF_BOUNDS] = int(FsError.Disk_OutOfBounds)
        for k in np.nonzero(status == STATUS_CORRECTED)[0]:
            self._log(int(ext["block"][k]))
        return err

    def read_extents(self, ext: np.ndarray, out: np.ndarray) -> np.ndarray:
        image = self._mapped_image()
        if image is None or not len(ext):
            return super().read_extents(ext, out)
        status = np.zeros(len(ext), dtype=np.uint8)
        wb = self._engine.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        self._engine.read_extents_host(image, np.ascontiguousarray(ext), out, status, write_back=wb)
        return self._extent_errors(ext, status)

    def write_extents(self, ext: np.ndarray, data: np.ndarray) -> np.ndarray:
        image = self._mapped_image()
        if image is None or not len(ext):
            return super().write_extents(ext, data)
        status = np.zeros(len(ext), dtype=np.uint8)
        self._engine.write_extents_host(data, image, np.ascontiguousarray(ext), status)
        return self._extent_errors(ext, status)

    def _file_engine_walk(self, image, file, first: int, count: int):
        """One engine walk of the tree on the mapped image: (image blocks, path statuses, the corrected blocks'
        events as (first file block under the index block, level, block))."""
        eng = self._engine
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        T = eng.file_tree_blocks(file, first, count)
        ix, ps = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint8)
        ti, ts = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint8)
        eng.file_blocks_host(image, file, first, count, ix, ps, ti, ts, write_back=wb)
        # the tree entries in level order (file_plan.hpp) with the first requested file block under each
        ipb, levels = self._ds // 4, [{}, {}, {}]
        for j in range(first, first + count):
            p = file_path_of(j, ipb)
            for d in range(p[0]):
                levels[d].setdefault(p[:d + 1], j)
        under = [(j, d) for d, lv in enumerate(levels) for j in lv.values()]
        events = [(j, d, int(ti[k])) for k, (j, d) in enumerate(under) if ts[k] == STATUS_CORRECTED]
        return ix, ps, events

    def _file_image(self, file, first: int, count: int):
        """The mapped image when the engine walks this range, None when the per-block loop does: no mapped disk, a
        shortened RS code, or a range the loop refuses partway."""
        image = self._mapped_image()
        f = np.asarray(file).reshape(-1)[0]
        if image is None or count <= 0 or self._ds == 0:
            return None
        if first + count > -(-int(f["file_size"]) // self._ds) or file_path_of(first + count - 1, self._ds // 4) is None:
            return None
        return image

    def file_blocks(self, file, first: int, count: int) -> Tuple[np.ndarray, Optional[FsError]]:
        """IBlockDevice.file_blocks in one engine call (EccEngine.file_blocks_host) on the disk image.  The result
        and the log up to the first failing index block equal the loop's; index blocks after it may additionally
        have been corrected and logged."""
        file = np.ascontiguousarray(file, dtype=FILE_DTYPE).reshape(1)
        image = self._file_image(file, first, count)
        if image is None:
            return super().file_blocks(file, first, count)
        ix, ps, events = self._file_engine_walk(image, file, first, count)
        for _, _, block in sorted(events, key=lambda e: e[:2]):
            self._log(block)
        bad = np.nonzero(ps)[0]
        if bad.size:
            return ix[:int(bad[0])].copy(), FsError(int(ps[bad[0]]))
        return ix, None

    def read_file(self, file, offset: int, bytes_to_read: int) -> Tuple[bytes, Optional[FsError]]:
        """IBlockDevice.read_file as engine calls on the disk image: the tree walk (EccEngine.file_blocks_host), then
        the blocks' byte ranges (EccEngine.read_extents_host).  The bytes, the error and the log up to the first
        failing block equal the loop's; blocks after it may additionally have been corrected and logged."""
        file = np.ascontiguousarray(file, dtype=FILE_DTYPE).reshape(1)
        size, ds = int(file["file_size"][0]), self._ds
        if bytes_to_read <= 0 or ds == 0 or offset >= size:
            return super().read_file(file, offset, bytes_to_read)
        n = min(bytes_to_read, size - offset)
        first, count = offset // ds, (offset % ds + n + ds - 1) // ds
        image = self._file_image(file, first, count)
        if image is None:
            return super().read_file(file, offset, bytes_to_read)
        ix, ps, events = self._file_engine_walk(image, file, first, count)
        live = np.nonzero(ps == 0)[0]
        ext = file_extents(ix, offset % ds, n, ds)
        out, st = np.zeros(n, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
        if live.size:
            st_live = np.zeros(live.size, dtype=np.uint8)
            wb = self._engine.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
            self._engine.read_extents_host(image, np.ascontiguousarray(ext[live]), out, st_live, write_back=wb)
            st[live] = st_live
        events += [(first + int(k), 3, int(ix[k])) for k in np.nonzero(st == STATUS_CORRECTED)[0]]
        for _, _, block in sorted(events, key=lambda e: e[:2]):
            self._log(block)
        final = np.where(ps != 0, ps, np.where(st == STATUS_CORRECTED, 0, st))
        bad = np.nonzero(final)[0]
        if bad.size:
            k = int(bad[0])
            return out[:int(ext["pos"][k])].tobytes(), FsError(int(final[k]))
        return out.tobytes(), None

    def read_files(self, files, ranges) -> List[Tuple[bytes, Optional[FsError]]]:
        """IBlockDevice.read_files as two engine calls on the disk image: one walk over all the files' trees
        (EccEngine.files_blocks_host), then the byte ranges of every block whose path held (EccEngine.read_extents_host).
        Per file the bytes, the error and the log up to the first failing block equal read_file's; files are logged in
        batch order; blocks after a file's failure may additionally have been corrected and logged."""
        files = np.ascontiguousarray(files, dtype=FILE_DTYPE).reshape(-1)
        ranges = [(int(off), int(n)) for off, n in ranges]
        image, ds = self._mapped_image(), self._ds
        if image is None or ds == 0 or len(ranges) != files.size:
            return super().read_files(files, ranges)
        results: List = [None] * files.size
        sel, spans = [], []
        for f, (off, want) in enumerate(ranges):
            size = int(files["file_size"][f])
            if want <= 0 or off >= size:  # answered from the range alone: no block is read
                results[f] = IBlockDevice.read_file(self, files[f:f + 1], off, want)
                continue
            n = min(want, size - off)
            first, count = off // ds, (off % ds + n + ds - 1) // ds
            if self._file_image(files[f:f + 1], first, count) is None:
                return super().read_files(files, ranges)  # a range the loop refuses partway: the loop is the definition
            sel.append(f)
            spans.append((off, n, first, count))
        if not sel:
            return results
        eng = self._engine
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        batch = np.ascontiguousarray(files[sel])
        byte_ranges = np.array([(off, n) for off, n, _, _ in spans], dtype=np.uint64).reshape(len(sel), 2)
        slots, totals = eng.files_plan(batch, byte_ranges)
        nb, T = int(totals["blocks"]), int(totals["tree_blocks"])
        ix, ps = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint8)
        ti, ts = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint8)
        eng.files_blocks_host(image, batch, byte_ranges, ix, ps, ti, ts, write_back=wb)
        ext = np.zeros(nb, dtype=EXTENT_DTYPE)
        for s, (off, n, _, count) in zip(slots, spans):
            at = int(s["block_pos"])
            e = file_extents(ix[at:at + count], off % ds, n, ds)
            e["pos"] += np.uint64(int(s["out_pos"]))
            ext[at:at + count] = e
        out, st = np.zeros(int(totals["bytes"]), dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
        live = np.nonzero(ps == 0)[0]
        if live.size:
            st_live = np.zeros(live.size, dtype=np.uint8)
            eng.read_extents_host(image, np.ascontiguousarray(ext[live]), out, st_live, write_back=wb)
            st[live] = st_live
        ipb = ds // 4
        for f, s, (off, n, first, count) in zip(sel, slots, spans):
            at, pos = int(s["block_pos"]), int(s["out_pos"])
            levels = [{}, {}, {}]  # the tree entries in level order with the first requested file block under each
            for j in range(first, first + count):
                p = file_path_of(j, ipb)
                for d in range(p[0]):
                    levels[d].setdefault(p[:d + 1], j)
            events = [(j, d, int(ti[int(s["tree_pos"][d]) + k])) for d, lv in enumerate(levels) for k, j in enumerate(lv.values())
                      if ts[int(s["tree_pos"][d]) + k] == STATUS_CORRECTED]
            f_ps, f_st = ps[at:at + count], st[at:at + count]
            events += [(first + int(k), 3, int(ix[at + k])) for k in np.nonzero(f_st == STATUS_CORRECTED)[0]]
            for _, _, block in sorted(events, key=lambda e: e[:2]):
                self._log(block)
            final = np.where(f_ps != 0, f_ps, np.where(f_st == STATUS_CORRECTED, 0, f_st))
            bad = np.nonzero(final)[0]
            if bad.size:
                k = int(bad[0])
                results[f] = (out[pos:int(ext["pos"][at + k])].tobytes(), FsError(int(final[k])))
            else:
                results[f] = (out[pos:pos + n].tobytes(), None)
        return results

    def _inode_log(self, t, nums, pieces) -> None:
        """The correction log of an inode call from its piece_status (rows of 1 + K slots), as the loop writes it:
        inodes in batch order, the bitmap block then the pieces up to the first failing one, each block that some
        access of the call corrected logged where the loop first touches it."""
        table_block, bitmap_block, ds = int(t["table_block"][0]), int(t["bitmap_block"][0]), self._ds
        touches = []  # per inode: (block, status) of the accesses the loop makes, in its order
        for i, ps in zip((int(x) for x in nums), pieces):
            mine = []
            if ps[0] != 255:
                mine.append((bitmap_block + (i // 8) // ds, int(ps[0])))
            for k, st in enumerate(ps[1:]):
                if st == 255:
                    break
                mine.append((table_block + 81 * i // ds + k, int(st)))
            touches.append(mine)
        corrected = {b for mine in touches for b, st in mine if st == STATUS_CORRECTED}
        logged = set()
        for mine in touches:
            for b, st in mine:
                if st in (STATUS_CORRECTION_ERROR, STATUS_OUT_OF_BOUNDS):
                    break
                if b in corrected and b not in logged:
                    logged.add(b)
                    self._log(b)

    @staticmethod
    def _inode_error(number: int, status: int, total: int) -> Optional[FsError]:
        """An inode call's status as the loop's result: None, or the loop's error."""
        if status in (STATUS_OK, STATUS_CORRECTED):
            return None
        if number >= total:
            return FsError.Bitmap_IndexOutOfRange
        return FsError.InodeManager_NotFound if status == STATUS_NOT_ALLOCATED else FsError(status)

    def read_inodes(self, table, numbers) -> List[Tuple[Optional[np.void], Optional[FsError]]]:
        """IBlockDevice.read_inodes as ONE engine call on the disk image (EccEngine.read_inodes_host).  Records and
        errors equal the loop's, and so does the correction log (_inode_log).  The pieces behind an inode's failing
        piece, which the loop does not read, have been read (and corrected) as well."""
        image = self._mapped_image()
        nums = np.ascontiguousarray(np.asarray(numbers).reshape(-1), dtype=np.uint32)
        if image is None or self._ds == 0 or self._ds > 0xFFFF or nums.size == 0:
            return super().read_inodes(table, numbers)
        eng = self._engine
        t = np.ascontiguousarray(np.asarray(table).reshape(-1)[:1], dtype=INODE_TABLE_DTYPE)
        n, W, total = int(nums.size), 1 + eng.inode_max_pieces, int(t["total_inodes"][0])
        files, meta = np.zeros(n, dtype=FILE_DTYPE), np.zeros(n, dtype=INODE_META_DTYPE)
        status, pieces = np.zeros(n, dtype=np.uint8), np.zeros(n * W, dtype=np.uint8)
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        eng.read_inodes_host(image, t, nums, files=files, meta=meta, status=status, piece_status=pieces, write_back=wb)
        self._inode_log(t, nums, pieces.reshape(n, W))
        out = []
        for j in range(n):
            error = self._inode_error(int(nums[j]), int(status[j]), total)
            rec = None
            if error is None:
                rec = np.zeros(1, dtype=INODE_DTYPE)
                rec["time_creation"], rec["time_modified"], rec["type"] = meta["time_creation"][j], meta["time_modified"][j], meta["type"][j]
                for name in FILE_DTYPE.names:
                    rec[name] = files[name][j]
                rec = rec[0]
            out.append((rec, error))
        return out

    def lookup(self, dirs, queries, names=None, mode: int = 0) -> List[Tuple[Optional[int], Optional[int], Optional[FsError]]]:
        """IBlockDevice.lookup as ONE EccEngine.lookup_host call on the disk image (after a walk without write-back,
        EccEngine.files_blocks_host, that tells which image block each file block and index block is, for the log).
        Results equal the loop's for every query.  The log holds the loop's events first and in the loop's order --
        queries in order, each block at its first read, an index block in front of the first file block under it.
        The engine reads every directory whole, so directory blocks that no query's loop reached -- behind last(B), or
        behind a failing block -- may additionally have been corrected: they are logged after the loop's events in
        (directory, block) order, and the disk is the loop's with exactly those blocks corrected as well."""
        image, ds = self._mapped_image(), self._ds
        dirs = np.ascontiguousarray(dirs, dtype=FILE_DTYPE).reshape(-1)
        q = np.ascontiguousarray(queries, dtype=LOOKUP_QUERY_DTYPE).reshape(-1)
        if image is None or ds == 0 or ds > 0xFFFF or q.size == 0 or int(q["dir"].max()) >= dirs.size:
            return super().lookup(dirs, queries, names, mode)
        eng = self._engine
        try:
            slots, totals = eng.lookup_plan(dirs)
        except EccError:  # a directory past its tree's capacity: the loop is the definition
            return super().lookup(dirs, queries, names, mode)
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        E, batch = self.DIR_ENTRY_BYTES, self.DIR_ENTRY_BATCH
        n_entries = dirs["file_size"].astype(np.int64) // E
        ranges = np.stack([np.zeros(dirs.size, np.uint64), (n_entries * E).astype(np.uint64)], axis=1)
        nb, T = int(totals["blocks"]), int(totals["tree_blocks"])
        ix, ps = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint8)
        ti, ts = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint8)
        if nb:
            eng.files_blocks_host(image, dirs, ranges, ix, ps, ti, ts, write_back=False)
        entries, bst = np.zeros(int(totals["bytes"]), dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
        nm = None if mode != 0 else np.ascontiguousarray(np.asarray(names, dtype=np.uint8).reshape(q.size, 128))
        hits, _, _ = eng.lookup_host(image, dirs, q, nm, mode, entries, bst, write_back=wb)
        # per directory, per file block: the tree entries above it, outermost first, as indices into ti / ts
        ipb, above = ds // 4, []
        for d, s in enumerate(slots):
            levels, rows = [{}, {}, {}], []
            for j in range(int(s["blocks"])):
                p = file_path_of(j, ipb)
                rows.append([int(s["tree_pos"][lv]) + levels[lv].setdefault(p[:lv + 1], len(levels[lv])) for lv in range(p[0])])
            above.append(rows)
        logged = set()

        def walk(d, upto):  # the reads of file blocks [0, upto] of directory d, until the first failing one
            at = int(slots[d]["block_pos"])
            for j in range(min(upto + 1, int(slots[d]["blocks"]))):
                for k in above[d][j]:
                    if ts[k] in (STATUS_CORRECTION_ERROR, STATUS_OUT_OF_BOUNDS):
                        return
                    if ts[k] == STATUS_CORRECTED and ("t", k) not in logged:
                        logged.add(("t", k))
                        self._log(int(ti[k]))
                if bst[at + j] in (STATUS_CORRECTION_ERROR, STATUS_OUT_OF_BOUNDS):
                    return
                if bst[at + j] == STATUS_CORRECTED and ("d", at + j) not in logged:
                    logged.add(("d", at + j))
                    self._log(int(ix[at + j]))

        out = []
        for h, d in zip(hits, (int(x) for x in q["dir"])):
            n, st = int(n_entries[d]), int(h["status"])
            if n:
                B = int(h["entry"]) // batch if st == STATUS_OK else (n - 1) // batch
                walk(d, (min((B + 1) * batch, n) * E - 1) // ds)
            if st == STATUS_OK:
                out.append((int(h["inode"]), int(h["entry"]), None))
            elif st == STATUS_NOT_FOUND:
                out.append((None, None, FsError.PpFS_NotFound if mode == 0 else FsError.DirectoryManager_NotFound))
            else:
                out.append((None, None, FsError(st)))
        if wb:  # what the engine corrected beyond the loop's reach
            for d, s in enumerate(slots):
                at = int(s["block_pos"])
                for j in range(int(s["blocks"])):
                    for k in above[d][j]:
                        if ts[k] == STATUS_CORRECTED and ("t", k) not in logged:
                            logged.add(("t", k))
                            self._log(int(ti[k]))
                    if bst[at + j] == STATUS_CORRECTED and ("d", at + j) not in logged:
                        logged.add(("d", at + j))
                        self._log(int(ix[at + j]))
        return out

    def write_inodes(self, table, numbers, files, meta) -> List[Optional[FsError]]:
        """IBlockDevice.write_inodes as ONE engine call on the disk image (EccEngine.write_inodes_host).  Errors equal
        the loop's, and so does the correction log (_inode_log).  The pieces behind an inode's failing piece, which the
        loop does not write, have been written as well."""
        image = self._mapped_image()
        nums = np.ascontiguousarray(np.asarray(numbers).reshape(-1), dtype=np.uint32)
        if image is None or self._ds == 0 or self._ds > 0xFFFF or nums.size == 0:
            return super().write_inodes(table, numbers, files, meta)
        eng = self._engine
        t = np.ascontiguousarray(np.asarray(table).reshape(-1)[:1], dtype=INODE_TABLE_DTYPE)
        n, W, total = int(nums.size), 1 + eng.inode_max_pieces, int(t["total_inodes"][0])
        rec = self._inode_pack(files, meta, n)  # checks the sizes
        f = np.zeros(n, dtype=FILE_DTYPE)
        m = np.zeros(n, dtype=INODE_META_DTYPE)
        for name in FILE_DTYPE.names:
            f[name] = rec[name]
        m["time_creation"], m["time_modified"], m["type"] = rec["time_creation"], rec["time_modified"], rec["type"]
        status, pieces = np.zeros(n, dtype=np.uint8), np.zeros(n * W, dtype=np.uint8)
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        eng.write_inodes_host(image, t, nums, f, m, status=status, piece_status=pieces, write_back=wb)
        self._inode_log(t, nums, pieces.reshape(n, W))
        return [self._inode_error(int(nums[j]), int(status[j]), total) for j in range(n)]

    def write_file(self, file, offset: int, data) -> Tuple[int, Optional[FsError]]:
        """IBlockDevice.write_file as write_files of one file."""
        file = np.ascontiguousarray(file, dtype=FILE_DTYPE).reshape(1)
        data = bytes(data)
        return self.write_files(file, [(offset, len(data))], [data])[0]

    def write_files(self, files, ranges, datas) -> List[Tuple[int, Optional[FsError]]]:
        """IBlockDevice.write_files as engine calls on the disk image: one walk over all the files' trees
        (EccEngine.files_blocks_host: which index blocks were corrected, for the log), then ONE
        EccEngine.write_files_host.  Per file `written`, the error and the log up to the first failing block equal
        write_file's; files are logged in batch order, index blocks in the order read_file uses.  Every block of every
        range is attempted: blocks after a file's failing block have been written (and logged) as well."""
        files = np.ascontiguousarray(files, dtype=FILE_DTYPE).reshape(-1)
        ranges = [(int(off), int(n)) for off, n in ranges]
        datas = [bytes(d) for d in datas]
        image, ds = self._mapped_image(), self._ds
        loop = lambda: [IBlockDevice.write_file(self, files[f:f + 1], off, datas[f][:max(n, 0)]) for f, (off, n) in enumerate(ranges)]
        if image is None or ds == 0 or len(ranges) != files.size or len(datas) != files.size:
            return loop()
        results: List = [None] * files.size
        sel, spans = [], []
        for f, (off, want) in enumerate(ranges):
            n = min(max(want, 0), len(datas[f]))
            if n == 0 or off < 0 or off + n > int(files["file_size"][f]):  # answered from the range alone: no block is touched
                results[f] = IBlockDevice.write_file(self, files[f:f + 1], off, datas[f][:n])
                continue
            first, count = off // ds, (off % ds + n + ds - 1) // ds
            if self._file_image(files[f:f + 1], first, count) is None:
                return loop()  # a range the loop refuses partway: the loop is the definition
            sel.append(f)
            spans.append((off, n, first, count))
        if not sel:
            return results
        eng = self._engine
        wb = eng.ecc_type in (ECC_REED_SOLOMON, ECC_HAMMING)
        batch = np.ascontiguousarray(files[sel])
        byte_ranges = np.array([(off, n) for off, n, _, _ in spans], dtype=np.uint64).reshape(len(sel), 2)
        slots, totals = eng.files_plan(batch, byte_ranges)
        nb, T = int(totals["blocks"]), int(totals["tree_blocks"])
        ix, ti, ts = np.zeros(nb, dtype=np.uint32), np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint8)
        eng.files_blocks_host(image, batch, byte_ranges, ix, None, ti, ts, write_back=wb)
        src = np.frombuffer(b"".join(datas[f][:n] for f, (_, n, _, _) in zip(sel, spans)), dtype=np.uint8)
        st = np.zeros(nb, dtype=np.uint8)
        _, written = eng.write_files_host(src, image, batch, byte_ranges, st, write_back=wb)
        ipb = ds // 4
        for k, (f, s, (off, n, first, count)) in enumerate(zip(sel, slots, spans)):
            at = int(s["block_pos"])
            levels = [{}, {}, {}]  # the tree entries in level order with the first requested file block under each
            for j in range(first, first + count):
                p = file_path_of(j, ipb)
                for d in range(p[0]):
                    levels[d].setdefault(p[:d + 1], j)
            events = [(j, d, int(ti[int(s["tree_pos"][d]) + q])) for d, lv in enumerate(levels) for q, j in enumerate(lv.values())
                      if ts[int(s["tree_pos"][d]) + q] == STATUS_CORRECTED]
            f_st = st[at:at + count]
            events += [(first + int(q), 3, int(ix[at + q])) for q in np.nonzero(f_st == STATUS_CORRECTED)[0]]
            for _, _, block in sorted(events, key=lambda e: e[:2]):
                self._log(block)
            bad = np.nonzero((f_st == STATUS_CORRECTION_ERROR) | (f_st == STATUS_OUT_OF_BOUNDS))[0]
            results[f] = (int(written[k]), FsError(int(f_st[bad[0]])) if bad.size else None)
        return results

    def readBlock(self, loc: DataLocation, bytes_to_read: int, capacity: Optional[int] = None) -> Expected[bytes]:
        if capacity is not None and capacity < bytes_to_read:
            return Expected.unexpected(FsError.Disk_InvalidRequest)
        to_read = min(self._ds - loc.offset, bytes_to_read)
        raw = self._read_raw(loc.block_index)
        if not raw:
            return Expected.unexpected(raw.error())
        dec = self._check_fix(loc.block_index, raw.value())
        if not dec:
            return Expected.unexpected(dec.error())
        return Expected(dec.value()[loc.offset:loc.offset + to_read].tobytes())

    def writeBlock(self, data, loc: DataLocation) -> Expected[int]:
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        to_write = min(data.size, self._ds - loc.offset)
        raw = self._read_raw(loc.block_index)
        if not raw:
            return Expected.unexpected(raw.error())
        raw = raw.value()
        dec = self._check_fix(loc.block_index, raw)
        if not dec:
            return Expected.unexpected(dec.error())
        payload = dec.value().copy()
        payload[loc.offset:loc.offset + to_write] = data[:to_write]
        self._engine.encode_host(payload, raw)  # raw: fixed old block (tail bits / parity byte base)
        w = self._disk.write(loc.block_index * self._raw, raw.tobytes())
        if not w:
            return Expected.unexpected(w.error())
        return Expected(int(to_write))


class ReedSolomonBlockDevice(_EngineDevice):  # rs_block_device.cpp
    _log_name = "ReedSolomon"

    def __init__(self, disk: IDisk, raw_block_size: int, correctable_bytes: int, logger: Optional[Logger] = None,
                 device: int = 0):
        super().__init__(EccEngine(ECC_REED_SOLOMON, raw_block_size, correctable_bytes, device=device), disk, logger)

    def _check_fix(self, block_index: int, raw: np.ndarray) -> Expected[np.ndarray]:
        e = self._engine
        data = np.zeros(self._ds, dtype=np.uint8)
        status = np.zeros(1, dtype=np.uint8)
        spill = np.zeros(e.spill_bytes_per_block(), dtype=np.uint8)
        fixed = raw.copy()
        e.decode_host(fixed, data, status, write_back=True, spill=spill)
        if status[0] == STATUS_CORRECTED:
            self._write_back(block_index, raw, fixed, spill)
        return Expected(data)

    def _write_back(self, block_index, old, fixed, spill) -> Optional[FsError]:
        self._log(block_index)  # :171-173
        extra = int(spill[0]) if (spill is not None and self._raw < 255) else 0
        wb = fixed.tobytes() + (spill[1:1 + extra].tobytes() if extra else b"")
        self._disk.write(block_index * self._raw, wb)  # result ignored (:180)
        return None

    def writeBlock(self, data, loc: DataLocation) -> Expected[int]:
        # the new codeword depends only on the patched payload (:61-93)
        return super().writeBlock(data, loc)


class CrcBlockDevice(_EngineDevice):  # crc_block_device.cpp
    def __init__(self, polynomial: CrcPolynomial, disk: IDisk, block_size: int, logger: Optional[Logger] = None,
                 device: int = 0):
        self.polynomial = polynomial
        super().__init__(EccEngine(ECC_CRC, block_size, crc_polynomial_explicit=polynomial.getExplicitPolynomial(),
                                   device=device), disk, logger)

    def _check_fix(self, block_index: int, raw: np.ndarray) -> Expected[np.ndarray]:
        data = np.zeros(self._ds, dtype=np.uint8)
        status = np.zeros(1, dtype=np.uint8)
        self._engine.decode_host(raw.copy(), data, status, write_back=False)
        if status[0] == STATUS_CORRECTION_ERROR:
            return Expected.unexpected(FsError.BlockDevice_CorrectionError)
        return Expected(data)

    def formatBlock(self, block_index: int) -> Expected[None]:
        # _calculateAndWrite on an all-zero block (:124-134)
        raw = np.zeros(self._raw, dtype=np.uint8)
        self._engine.encode_host(np.zeros(self._ds, dtype=np.uint8), raw)
        r = self._disk.write(block_index * self._raw, raw.tobytes())
        return Expected(None) if r else Expected.unexpected(r.error())


class HammingBlockDevice(_EngineDevice):  # hamming_block_device.cpp
    _log_name = "Hamming"

    def __init__(self, block_size_power: int, disk: IDisk, logger: Optional[Logger] = None, device: int = 0):
        super().__init__(EccEngine(ECC_HAMMING, 1 << int(block_size_power), device=device), disk, logger)

    def _check_fix(self, block_index: int, raw: np.ndarray) -> Expected[np.ndarray]:
        data = np.zeros(self._ds, dtype=np.uint8)
        status = np.zeros(1, dtype=np.uint8)
        fixed = raw.copy()
        self._engine.decode_host(fixed, data, status, write_back=True)
        if status[0] == STATUS_CORRECTION_ERROR:
            return Expected.unexpected(FsError.BlockDevice_CorrectionError)
        if status[0] == STATUS_CORRECTED:
            fe = self._write_back(block_index, raw, fixed, None)
            if fe is not None:
                return Expected.unexpected(fe)
            raw[:] = fixed
        return Expected(data)

    def _write_back(self, block_index, old, fixed, spill) -> Optional[FsError]:
        diff = np.nonzero(fixed != old)[0]
        byte = int(diff[0]) if diff.size else 0
        w = self._disk.write(block_index * self._raw + byte, fixed[byte:byte + 1].tobytes())  # :41-51
        if not w:
            return w.error()
        self._log(block_index)  # :53-57
        return None


class ParityBlockDevice(_EngineDevice):  # parity_block_device.cpp
    def __init__(self, block_size: int, disk: IDisk, logger: Optional[Logger] = None, device: int = 0):
        super().__init__(EccEngine(ECC_PARITY, block_size, device=device), disk, logger)

    def _check_fix(self, block_index: int, raw: np.ndarray) -> Expected[np.ndarray]:
        data = np.zeros(self._ds, dtype=np.uint8)
        status = np.zeros(1, dtype=np.uint8)
        self._engine.decode_host(raw.copy(), data, status, write_back=False)
        if status[0] == STATUS_CORRECTION_ERROR:
            return Expected.unexpected(FsError.BlockDevice_CorrectionError)
        return Expected(data)


def create_block_device(disk: IDisk, block_size: int, ecc_type: ECCType, crc_polynomial_explicit: int = 0,
                        rs_correctable_bytes: int = 3, logger: Optional[Logger] = None,
                        device: int = 0) -> IBlockDevice:
    """PpFS::_createAppropriateBlockDevice (lib/filesystem/src/ppfs.cpp:35-70)."""
    t = ECCType(ecc_type)
    if t == ECCType.None_:
        return RawBlockDevice(block_size, disk)
    if t == ECCType.Parity:
        return ParityBlockDevice(block_size, disk, logger, device)
    if t == ECCType.Crc:
        return CrcBlockDevice(CrcPolynomial.MsgExplicit(crc_polynomial_explicit), disk, block_size, logger, device)
    if t == ECCType.Hamming:
        return HammingBlockDevice(int(math.log2(block_size)), disk, logger, device)
    return ReedSolomonBlockDevice(disk, block_size, rs_correctable_bytes, logger, device)
