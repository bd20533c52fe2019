"""EccEngine: one codec context on one GPU (wraps ppfs_ecc_ctx from include/ppfs_ecc.h).

Device-resident calls take torch uint8 CUDA tensors (HBM buffers, packed blocks) and enqueue
the HIP kernels on the current torch stream; host calls take numpy uint8 arrays and go through
the library's pinned, double-buffered staging.  torch is used only as the HBM allocator and
stream provider.
"""
from __future__ import annotations

import collections
import ctypes
from ctypes import byref, c_void_p
from typing import Optional

import numpy as np

from . import _native
from ._native import EccParams, check, lib


def _ptr(x) -> Optional[int]:
    """Device/host address of a torch tensor or numpy array (None passes NULL)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"] or x.dtype != np.uint8:
            raise ValueError("numpy buffers must be C-contiguous uint8")
        return x.ctypes.data
    # torch tensor
    if not x.is_contiguous() or x.element_size() != 1:
        raise ValueError("tensors must be contiguous uint8")
    return x.data_ptr()


def _size(x) -> int:
    """Bytes of a uint8 buffer (numpy array or torch tensor)."""
    return int(x.size) if isinstance(x, np.ndarray) else int(x.numel())


def _need(name: str, x, nbytes: int, kind: str) -> None:
    """Reject a buffer shorter than the call will touch (the library trusts its sizes: a short
    host array would overflow the heap, a short tensor would be written out of bounds in HBM),
    and a buffer of the wrong memory kind for the entry point."""
    if x is None:
        return
    if kind == "device":
        if isinstance(x, np.ndarray) or not getattr(x, "is_cuda", False):
            raise ValueError(f"{name}: device entry points take CUDA tensors")
    elif not isinstance(x, np.ndarray):
        raise ValueError(f"{name}: host entry points take numpy arrays")
    if _size(x) < nbytes:
        raise ValueError(f"{name}: {_size(x)} bytes < {nbytes} needed")


def _host_blocks(x, per_block: int, name: str) -> int:
    """Blocks a host array holds (the block count the *_host calls take from it)."""
    if not isinstance(x, np.ndarray):
        raise ValueError(f"{name}: host entry points take numpy arrays")
    return x.size // per_block


def _stream_handle(stream) -> Optional[int]:
    if stream is not None:
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    import torch

    return torch.cuda.current_stream().cuda_stream


class EccEngine:
    """Codec context: params follow PpFS::_createAppropriateBlockDevice (ppfs.cpp:35-70)."""

    def __init__(self, ecc_type: int, block_size: int, rs_correctable_bytes: int = 3,
                 crc_polynomial_explicit: int = 0, device: int = 0):
        p = EccParams(int(ecc_type), int(block_size), int(rs_correctable_bytes), 0, int(crc_polynomial_explicit))
        h = c_void_p()
        check(lib().ppfs_ecc_create(byref(p), int(device), byref(h)))
        self._h = h
        self.ecc_type = int(ecc_type)
        self.block_size = int(block_size)
        self.device = int(device)
        self.raw_block_size = int(lib().ppfs_ecc_raw_block_size(h))
        self.data_size = int(lib().ppfs_ecc_data_size(h))
        self.kernel_name = lib().ppfs_ecc_kernel_name(h).decode()

    def stream_kernel_name(self, stream=None) -> str:
        """The kernel path a device call on `stream` (default: torch's current stream) takes
        (ppfs_ecc_stream_kernel_name): kernel_name, except that RS 2t <= 8 runs its static-walk
        kernels on a 17th distinct stream and on a stream capturing a graph."""
        return lib().ppfs_ecc_stream_kernel_name(self._h, _stream_handle(stream)).decode()

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ppfs_ecc_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------- device-resident batches (torch CUDA uint8 tensors) ----------------
    def _check(self, kind, n, data=None, raw=None, status=None, spill=None) -> None:
        if n < 0:
            raise ValueError("nblocks must be >= 0")
        _need("data", data, n * self.data_size, kind)
        _need("raw", raw, n * self.raw_block_size, kind)
        _need("status", status, n, kind)
        _need("spill", spill, n * self.spill_bytes_per_block(), kind)

    def _nblocks(self, data, raw) -> int:
        """Blocks a call covers when nblocks is not given: from the payloads, or from the raw
        blocks for codecs without payload bytes (Hamming power 0, 1-byte parity blocks)."""
        return _size(data) // self.data_size if self.data_size else _size(raw) // self.raw_block_size

    def encode(self, data, raw, nblocks: Optional[int] = None, stream=None) -> None:
        n = nblocks if nblocks is not None else self._nblocks(data, raw)
        self._check("device", n, data, raw)
        check(lib().ppfs_ecc_encode_device(self._h, _ptr(data), _ptr(raw), n, _stream_handle(stream)))

    def decode(self, raw, data=None, status=None, write_back: bool = True, spill=None,
               nblocks: Optional[int] = None, stream=None) -> None:
        n = nblocks if nblocks is not None else raw.numel() // self.raw_block_size
        self._check("device", n, data, raw, status, spill)
        check(lib().ppfs_ecc_decode_device(self._h, _ptr(raw), _ptr(data), _ptr(status), n, int(bool(write_back)),
                                           _ptr(spill), _stream_handle(stream)))

    def write(self, data, raw, status=None, nblocks: Optional[int] = None, stream=None) -> None:
        n = nblocks if nblocks is not None else self._nblocks(data, raw)
        self._check("device", n, data, raw, status)
        check(lib().ppfs_ecc_write_device(self._h, _ptr(data), _ptr(raw), _ptr(status), n,
                                          _stream_handle(stream)))

    # ---------------- host-memory batches (numpy uint8) ----------------
    def encode_host(self, data: np.ndarray, raw: np.ndarray) -> None:
        n = _host_blocks(data, self.data_size, "data") if self.data_size else _host_blocks(raw, self.raw_block_size, "raw")
        self._check("host", n, data, raw)
        check(lib().ppfs_ecc_encode_host(self._h, _ptr(data), _ptr(raw), n))

    def decode_host(self, raw: np.ndarray, data: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None,
                    write_back: bool = True, spill: Optional[np.ndarray] = None) -> None:
        n = _host_blocks(raw, self.raw_block_size, "raw")
        self._check("host", n, data, raw, status, spill)
        check(lib().ppfs_ecc_decode_host(self._h, _ptr(raw), _ptr(data), _ptr(status), n, int(bool(write_back)),
                                         _ptr(spill)))

    def write_host(self, data: np.ndarray, raw: np.ndarray, status: Optional[np.ndarray] = None) -> None:
        n = _host_blocks(data, self.data_size, "data") if self.data_size else _host_blocks(raw, self.raw_block_size, "raw")
        self._check("host", n, data, raw, status)
        check(lib().ppfs_ecc_write_host(self._h, _ptr(data), _ptr(raw), _ptr(status), n))

    def host_chunk_blocks(self) -> int:
        """Blocks per staging chunk of the *_host calls (ppfs_ecc_host_chunk_blocks)."""
        return int(lib().ppfs_ecc_host_chunk_blocks(self._h))

    def spill_bytes_per_block(self) -> int:
        return 256 - min(self.raw_block_size, 255)

    # ---------------- block lists (include/ppfs_ecc.h ppfs_ecc_*_list_*) ----------------
    # "these block indices of this image, in this order": entry i is block index[i] of the image;
    # payloads, statuses and spill records are in list order.  An index past the image gets status 9
    # (STATUS_OUT_OF_BOUNDS) and a zero payload.  The image's block count is taken from its size.
    def _list_check(self, kind, image, index, data=None, status=None, spill=None):
        """(entries, image blocks) of a list call after the buffer checks of the contiguous calls."""
        if kind == "device":
            import torch

            if isinstance(index, np.ndarray) or not getattr(index, "is_cuda", False):
                raise ValueError("index: device entry points take CUDA tensors")
            if index.dtype != torch.int32 or not index.is_contiguous() or index.dim() != 1:
                raise ValueError("index: a contiguous 1-D torch.int32 tensor (read as unsigned)")
            n = int(index.numel())
        else:
            if not isinstance(index, np.ndarray):
                raise ValueError("index: host entry points take numpy arrays")
            if index.dtype != np.uint32 or not index.flags["C_CONTIGUOUS"] or index.ndim != 1:
                raise ValueError("index: a C-contiguous 1-D numpy uint32 array")
            n = int(index.size)
        if image is None:
            raise ValueError("image: required")
        _need("image", image, 0, kind)
        _ptr(image)  # contiguous uint8
        self._check(kind, n, data=data, status=status, spill=spill)
        return n, _size(image) // self.raw_block_size

    @staticmethod
    def _index_ptr(index) -> int:
        return index.ctypes.data if isinstance(index, np.ndarray) else index.data_ptr()

    def _list_payload(self, kind, data, n) -> None:
        if data is None and self.data_size and n:
            raise ValueError("data: required")
        _need("data", data, n * self.data_size, kind)

    def list_kernel_name(self) -> str:
        """How decode_list runs (ppfs_ecc_list_kernel_name): "rs255-wg-list-lds", one kernel that fetches
        the listed rows itself (RS bs >= 255, t <= 4), or "gather-stage-scatter", the staged pipeline."""
        return lib().ppfs_ecc_list_kernel_name(self._h).decode()

    def list_encode_kernel_name(self) -> str:
        """How encode_list and write_list run (ppfs_ecc_list_encode_kernel_name): "rs255-wg-list-store-lds",
        one kernel that stores each codeword at its row of the image (RS bs >= 255, t <= 4), or
        "gather-stage-scatter", the staged pipeline."""
        return lib().ppfs_ecc_list_encode_kernel_name(self._h).decode()

    def decode_list(self, image, index, data=None, status=None, write_back: bool = True, spill=None, stream=None) -> None:
        n, blocks = self._list_check("device", image, index, data, status, spill)
        check(lib().ppfs_ecc_decode_list_device(self._h, _ptr(image), blocks, self._index_ptr(index), n, _ptr(data),
                                                _ptr(status), int(bool(write_back)), _ptr(spill),
                                                _stream_handle(stream)))

    def encode_list(self, data, image, index, stream=None) -> None:
        n, blocks = self._list_check("device", image, index, data)
        self._list_payload("device", data, n)
        check(lib().ppfs_ecc_encode_list_device(self._h, _ptr(data), _ptr(image), blocks, self._index_ptr(index), n,
                                                _stream_handle(stream)))

    def write_list(self, data, image, index, status=None, stream=None) -> None:
        n, blocks = self._list_check("device", image, index, data, status)
        self._list_payload("device", data, n)
        check(lib().ppfs_ecc_write_list_device(self._h, _ptr(data), _ptr(image), blocks, self._index_ptr(index),
                                               _ptr(status), n, _stream_handle(stream)))

    def decode_list_host(self, image: np.ndarray, index: np.ndarray, data: Optional[np.ndarray] = None,
                         status: Optional[np.ndarray] = None, write_back: bool = True,
                         spill: Optional[np.ndarray] = None) -> None:
        n, blocks = self._list_check("host", image, index, data, status, spill)
        check(lib().ppfs_ecc_decode_list_host(self._h, _ptr(image), blocks, self._index_ptr(index), n, _ptr(data),
                                              _ptr(status), int(bool(write_back)), _ptr(spill)))

    def encode_list_host(self, data: np.ndarray, image: np.ndarray, index: np.ndarray) -> None:
        n, blocks = self._list_check("host", image, index, data)
        self._list_payload("host", data, n)
        check(lib().ppfs_ecc_encode_list_host(self._h, _ptr(data), _ptr(image), blocks, self._index_ptr(index), n))

    def write_list_host(self, data: np.ndarray, image: np.ndarray, index: np.ndarray,
                        status: Optional[np.ndarray] = None) -> None:
        n, blocks = self._list_check("host", image, index, data, status)
        self._list_payload("host", data, n)
        check(lib().ppfs_ecc_write_list_host(self._h, _ptr(data), _ptr(image), blocks, self._index_ptr(index),
                                             _ptr(status), n))

    # ---------------- byte extents (include/ppfs_ecc.h ppfs_ecc_*_extents_*) ----------------
    # "these byte ranges of those blocks": entry i (_native.EXTENT_DTYPE: pos, block, offset, length) is
    # readBlock({block, offset}, length) / writeBlock(bytes, {block, offset}); its bytes lie at
    # [pos, pos + min(length, data_size - offset)) of the packed buffer.  An invalid entry gets status 9.
    def _extents(self, kind, ext):
        """(extents as the call takes them, entries): a numpy EXTENT_DTYPE array (host calls; device
        calls copy it to the GPU) or, for device calls, a CUDA uint8 tensor of 16 bytes per entry."""
        if isinstance(ext, np.ndarray):
            if ext.dtype != _native.EXTENT_DTYPE or ext.ndim != 1 or not ext.flags["C_CONTIGUOUS"]:
                raise ValueError("extents: a C-contiguous 1-D numpy array of EXTENT_DTYPE")
            return ext, int(ext.size)
        if kind != "device":
            raise ValueError("extents: host entry points take a numpy array of EXTENT_DTYPE")
        import torch

        if not getattr(ext, "is_cuda", False) or ext.dtype != torch.uint8 or not ext.is_contiguous() or ext.dim() != 1 \
                or ext.numel() % 16 or ext.data_ptr() % 8:
            raise ValueError("extents: a contiguous 1-D CUDA uint8 tensor of 16 bytes per entry, 8-byte aligned")
        return ext, int(ext.numel()) // 16

    def _extent_check(self, kind, image, ext, buf, status):
        """(extents, entries, image blocks, bytes of the packed buffer) after the buffer checks."""
        ext, n = self._extents(kind, ext)
        if image is None:
            raise ValueError("image: required")
        _need("image", image, 0, kind)
        _need("buffer", buf, 0, kind)
        _need("status", status, n, kind)
        _ptr(image), _ptr(buf), _ptr(status)  # contiguous uint8
        if kind == "device" and isinstance(ext, np.ndarray):
            import torch

            ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
            self._ext_keep = ext  # the queued kernels read it: alive until the next such call
        return ext, n, _size(image) // self.raw_block_size, 0 if buf is None else _size(buf)

    def read_extents(self, image, ext, out, status=None, write_back: bool = True, stream=None) -> None:
        ext, n, blocks, nbytes = self._extent_check("device", image, ext, out, status)
        check(lib().ppfs_ecc_read_extents_device(self._h, _ptr(image), blocks, self._index_ptr(ext), n, _ptr(out), nbytes,
                                                 _ptr(status), int(bool(write_back)), _stream_handle(stream)))

    def write_extents(self, data, image, ext, status=None, stream=None) -> None:
        ext, n, blocks, nbytes = self._extent_check("device", image, ext, data, status)
        check(lib().ppfs_ecc_write_extents_device(self._h, _ptr(data), nbytes, _ptr(image), blocks, self._index_ptr(ext), n,
                                                  _ptr(status), _stream_handle(stream)))

    def read_extents_host(self, image: np.ndarray, ext: np.ndarray, out: Optional[np.ndarray],
                          status: Optional[np.ndarray] = None, write_back: bool = True) -> None:
        ext, n, blocks, nbytes = self._extent_check("host", image, ext, out, status)
        check(lib().ppfs_ecc_read_extents_host(self._h, _ptr(image), blocks, self._index_ptr(ext), n, _ptr(out), nbytes,
                                               _ptr(status), int(bool(write_back))))

    def write_extents_host(self, data: Optional[np.ndarray], image: np.ndarray, ext: np.ndarray,
                           status: Optional[np.ndarray] = None) -> None:
        ext, n, blocks, nbytes = self._extent_check("host", image, ext, data, status)
        check(lib().ppfs_ecc_write_extents_host(self._h, _ptr(data), nbytes, _ptr(image), blocks, self._index_ptr(ext), n,
                                                _ptr(status)))

    # ---------------- whole-image scrub ----------------
    def scrub_host(self, image: np.ndarray, nblocks: Optional[int] = None, status: Optional[np.ndarray] = None):
        """readBlock(i) for every block of a host image, in order, for its write-back effect only
        (include/ppfs_ecc.h ppfs_ecc_scrub_host).  Returns (ok, corrected, failed) block counts."""
        n = nblocks if nblocks is not None else _host_blocks(image, self.raw_block_size, "image")
        self._check("host", n, raw=image, status=status)
        counts = (ctypes.c_size_t * 3)()
        check(lib().ppfs_ecc_scrub_host(self._h, _ptr(image), image.size, n, _ptr(status), counts))
        return int(counts[0]), int(counts[1]), int(counts[2])

    def scrub(self, image, status=None, nblocks: Optional[int] = None, stream=None) -> None:
        """Device-resident scrub of a torch uint8 image (ppfs_ecc_scrub_device)."""
        n = nblocks if nblocks is not None else image.numel() // self.raw_block_size
        self._check("device", n, raw=image, status=status)
        check(lib().ppfs_ecc_scrub_device(self._h, _ptr(image), image.numel(), n, _ptr(status),
                                          _stream_handle(stream)))

    # ---------------- scrub of named blocks (ppfs_ecc_scrub_list_*, ppfs_ecc_scrub_allocated_*) ----------------
    # A list scrub is decode_list(data=None, write_back=True) plus counts; an allocated scrub reads the
    # reference's on-disk bitmap as it lies in the image (bit j of the bitmap starting at block
    # bitmap_block stands for block first_block + j) and list-scrubs the blocks whose bit is set.
    @staticmethod
    def _device_counts(counts):
        """The 64-byte device record of a device scrub: None, True (a fresh tensor) or the caller's tensor of
        eight int64."""
        if counts is None or counts is False:
            return None
        import torch

        if counts is True:
            return torch.zeros(8, dtype=torch.int64, device="cuda")
        if not getattr(counts, "is_cuda", False) or counts.dtype != torch.int64 or not counts.is_contiguous() \
                or counts.numel() < 8:
            raise ValueError("counts: a contiguous CUDA int64 tensor of 8 elements (fields of SCRUB_COUNT_FIELDS)")
        return counts

    def bitmap_blocks(self, nbits: int) -> int:
        """Blocks a bitmap of nbits bits spans (Bitmap::blocksSpanned, in integer arithmetic)."""
        if not self.data_size:
            raise ValueError("blocks of this codec have no payload")
        return -(-(-(-int(nbits) // 8)) // self.data_size)

    def scrub_list(self, image, index, status=None, counts=None, stream=None):
        """Device list scrub.  counts: None, True (returns a fresh CUDA int64 tensor of the eight fields of
        SCRUB_COUNT_FIELDS; read it after synchronising) or such a tensor of the caller's.  Never synchronises."""
        n, blocks = self._list_check("device", image, index, status=status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_scrub_list_device(self._h, _ptr(image), blocks, self._index_ptr(index), n, _ptr(status),
                                               None if d_counts is None else d_counts.data_ptr(),
                                               _stream_handle(stream)))
        return d_counts

    def scrub_list_host(self, image: np.ndarray, index: np.ndarray, status: Optional[np.ndarray] = None) -> "ScrubCounts":
        n, blocks = self._list_check("host", image, index, status=status)
        rec = _native.ScrubCounts()
        check(lib().ppfs_ecc_scrub_list_host(self._h, _ptr(image), blocks, self._index_ptr(index), n, _ptr(status),
                                             byref(rec)))
        return ScrubCounts(*[int(getattr(rec, f)) for f in SCRUB_COUNT_FIELDS])

    def _allocated_check(self, kind, image, nbits, status, bitmap_status):
        if image is None:
            raise ValueError("image: required")
        if nbits < 0:
            raise ValueError("nbits must be >= 0")
        _need("image", image, 0, kind)
        _need("status", status, nbits, kind)
        _need("bitmap_status", bitmap_status, self.bitmap_blocks(nbits), kind)
        _ptr(image), _ptr(status), _ptr(bitmap_status)  # contiguous uint8
        return _size(image) // self.raw_block_size

    def scrub_allocated(self, image, bitmap_block: int, first_block: int, nbits: int, status=None, bitmap_status=None,
                        counts=None, stream=None):
        """Device allocated scrub; counts as in scrub_list.  Synchronises the stream once per 1 Mi bits."""
        blocks = self._allocated_check("device", image, nbits, status, bitmap_status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_scrub_allocated_device(self._h, _ptr(image), blocks, int(bitmap_block), int(first_block),
                                                    int(nbits), _ptr(status), _ptr(bitmap_status),
                                                    None if d_counts is None else d_counts.data_ptr(),
                                                    _stream_handle(stream)))
        return d_counts

    def scrub_allocated_host(self, image: np.ndarray, bitmap_block: int, first_block: int, nbits: int,
                             status: Optional[np.ndarray] = None,
                             bitmap_status: Optional[np.ndarray] = None) -> "ScrubCounts":
        blocks = self._allocated_check("host", image, nbits, status, bitmap_status)
        rec = _native.ScrubCounts()
        check(lib().ppfs_ecc_scrub_allocated_host(self._h, _ptr(image), blocks, int(bitmap_block), int(first_block),
                                                  int(nbits), _ptr(status), _ptr(bitmap_status), byref(rec)))
        return ScrubCounts(*[int(getattr(rec, f)) for f in SCRUB_COUNT_FIELDS])

    # ---------------- read a file from its inode (ppfs_ecc_file_*, ppfs_ecc_read_file_*) ----------------
    # `file` is the 64-byte record of _native.FILE_DTYPE (direct[12], indirect, doubly_indirect, trebly_indirect,
    # file_size), always in host memory.  The walk resolves the index-block tree on the GPU: at most three list
    # decodes with an expansion between them; read_file then reads the range like FileIO::readFile.
    @staticmethod
    def _file(file) -> np.ndarray:
        f = np.ascontiguousarray(file)
        if f.dtype != _native.FILE_DTYPE or f.size != 1:
            raise ValueError("file: one record of FILE_DTYPE")
        return f.reshape(1)

    def file_span(self, file, offset: int, nbytes: int):
        """(first file block, blocks, bytes delivered) of readFile(offset, nbytes) (ppfs_ecc_file_span)."""
        f = self._file(file)
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().ppfs_ecc_file_span(self._h, f.ctypes.data, int(offset), int(nbytes), byref(a), byref(b), byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def file_tree_blocks(self, file, first_block: int, nblocks: int) -> int:
        """Index blocks a walk over [first_block, first_block + nblocks) visits (ppfs_ecc_file_tree_blocks)."""
        f = self._file(file)
        t = int(lib().ppfs_ecc_file_tree_blocks(self._h, f.ctypes.data, int(first_block), int(nblocks)))
        if t < 0:
            check(t)
        return t

    def _file_blocks_check(self, kind, image, file, first_block, nblocks, index, path_status, tree_index, tree_status):
        f = self._file(file)
        if image is None:
            raise ValueError("image: required")
        if first_block < 0 or nblocks < 0:
            raise ValueError("first_block and nblocks must be >= 0")
        t = self.file_tree_blocks(f, first_block, nblocks)
        _need("image", image, 0, kind)
        _need("path_status", path_status, nblocks, kind)
        _need("tree_status", tree_status, t, kind)
        _ptr(image), _ptr(path_status), _ptr(tree_status)  # contiguous uint8
        for name, x, n in (("index", index, nblocks), ("tree_index", tree_index, t)):
            if x is None:
                continue
            if kind == "device":
                import torch

                if isinstance(x, np.ndarray) or not getattr(x, "is_cuda", False) or x.dtype != torch.int32 \
                        or not x.is_contiguous() or x.dim() != 1 or x.numel() < n:
                    raise ValueError(f"{name}: a contiguous 1-D CUDA torch.int32 tensor of >= {n} elements (read as unsigned)")
            elif not isinstance(x, np.ndarray) or x.dtype != np.uint32 or not x.flags["C_CONTIGUOUS"] or x.ndim != 1 \
                    or x.size < n:
                raise ValueError(f"{name}: a C-contiguous 1-D numpy uint32 array of >= {n} elements")
        return f, _size(image) // self.raw_block_size

    def file_blocks(self, image, file, first_block: int, nblocks: int, index=None, path_status=None, tree_index=None,
                    tree_status=None, counts=None, write_back: bool = True, stream=None):
        """Device walk (ppfs_ecc_file_blocks_device).  counts: None, True (returns a fresh CUDA int64 tensor of the
        eight fields of FILE_COUNT_FIELDS; read it after synchronising) or such a tensor.  Never synchronises."""
        f, blocks = self._file_blocks_check("device", image, file, first_block, nblocks, index, path_status, tree_index,
                                            tree_status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_file_blocks_device(
            self._h, _ptr(image), blocks, f.ctypes.data, int(first_block), int(nblocks),
            None if index is None else self._index_ptr(index), _ptr(path_status),
            None if tree_index is None else self._index_ptr(tree_index), _ptr(tree_status),
            None if d_counts is None else d_counts.data_ptr(), int(bool(write_back)), _stream_handle(stream)))
        return d_counts

    def file_blocks_host(self, image: np.ndarray, file, first_block: int, nblocks: int, index=None, path_status=None,
                         tree_index=None, tree_status=None, write_back: bool = True) -> "FileCounts":
        f, blocks = self._file_blocks_check("host", image, file, first_block, nblocks, index, path_status, tree_index,
                                            tree_status)
        rec = _native.FileCounts()
        check(lib().ppfs_ecc_file_blocks_host(
            self._h, _ptr(image), blocks, f.ctypes.data, int(first_block), int(nblocks),
            None if index is None else self._index_ptr(index), _ptr(path_status),
            None if tree_index is None else self._index_ptr(tree_index), _ptr(tree_status), byref(rec),
            int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, n)) for n in FILE_COUNT_FIELDS])

    def _read_file_check(self, kind, image, file, offset, nbytes, out, status):
        f = self._file(file)
        if image is None:
            raise ValueError("image: required")
        if offset < 0 or nbytes < 0:
            raise ValueError("offset and nbytes must be >= 0")
        _, nblocks, clamped = self.file_span(f, offset, nbytes)
        _need("image", image, 0, kind)
        _need("out", out, clamped, kind)
        _need("status", status, nblocks, kind)
        _ptr(image), _ptr(out), _ptr(status)  # contiguous uint8
        return f, _size(image) // self.raw_block_size, 0 if out is None else _size(out)

    def read_file(self, image, file, offset: int, nbytes: int, out, status=None, counts=None, write_back: bool = True,
                  stream=None):
        """Device file read (ppfs_ecc_read_file_device): out[0, clamped) = the file range; status: one byte per file
        block touched; counts as in file_blocks.  Never synchronises."""
        f, blocks, out_bytes = self._read_file_check("device", image, file, offset, nbytes, out, status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_read_file_device(self._h, _ptr(image), blocks, f.ctypes.data, int(offset), int(nbytes), _ptr(out),
                                              out_bytes, _ptr(status), None if d_counts is None else d_counts.data_ptr(),
                                              int(bool(write_back)), _stream_handle(stream)))
        return d_counts

    def read_file_host(self, image: np.ndarray, file, offset: int, nbytes: int, out: Optional[np.ndarray],
                       status: Optional[np.ndarray] = None, write_back: bool = True) -> "FileCounts":
        f, blocks, out_bytes = self._read_file_check("host", image, file, offset, nbytes, out, status)
        rec = _native.FileCounts()
        check(lib().ppfs_ecc_read_file_host(self._h, _ptr(image), blocks, f.ctypes.data, int(offset), int(nbytes), _ptr(out),
                                            out_bytes, _ptr(status), byref(rec), int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, n)) for n in FILE_COUNT_FIELDS])

    # ---------------- read many files in one call (ppfs_ecc_files_*, ppfs_ecc_read_files_*) ----------------
    # `files` is a FILE_DTYPE array of any length in host memory, `ranges` None (every file whole) or an (n, 2) uint64
    # array of (offset, nbytes).  files_plan says where each file's results lie in the batch's arrays: per-block arrays
    # and out hold the files back to back, the tree arrays are level-major.  file_flags: one uint32 per file.
    @staticmethod
    def _files(files, ranges):
        f = np.ascontiguousarray(files)
        if f.dtype != _native.FILE_DTYPE or f.ndim > 1:
            raise ValueError("files: a 1-D array of FILE_DTYPE records")
        f = f.reshape(-1)
        if ranges is None:
            return f, None
        r = np.ascontiguousarray(ranges)
        if r.dtype != np.uint64 or r.shape != (f.size, 2):
            raise ValueError(f"ranges: None or a ({f.size}, 2) numpy uint64 array of (offset, nbytes)")
        return f, r

    def files_plan(self, files, ranges=None):
        """(slots, totals) of a batch (ppfs_ecc_files_plan): one FILES_SLOT_DTYPE record per file and one
        FILES_TOTALS_DTYPE record.  No GPU work."""
        f, r = self._files(files, ranges)
        slots, totals = np.zeros(f.size, _native.FILES_SLOT_DTYPE), np.zeros(1, _native.FILES_TOTALS_DTYPE)
        check(lib().ppfs_ecc_files_plan(self._h, f.ctypes.data if f.size else None, None if r is None else r.ctypes.data,
                                        f.size, slots.ctypes.data if f.size else None, totals.ctypes.data))
        return slots, totals[0]

    def _files_check(self, kind, image, files, ranges, index=None, path_status=None, tree_index=None, tree_status=None,
                     file_flags=None, out=None, status=None, read=False):
        f, r = self._files(files, ranges)
        if image is None:
            raise ValueError("image: required")
        _, totals = self.files_plan(f, r)
        nblocks, t = int(totals["blocks"]), int(totals["tree_blocks"])
        _need("image", image, 0, kind)
        _need("path_status", path_status, nblocks, kind)
        _need("tree_status", tree_status, t, kind)
        _need("status", status, nblocks, kind)
        if read:
            _need("out", out, int(totals["bytes"]), kind)
        _ptr(image), _ptr(path_status), _ptr(tree_status), _ptr(status), _ptr(out)  # contiguous uint8
        for name, x, n in (("index", index, nblocks), ("tree_index", tree_index, t), ("file_flags", file_flags, f.size)):
            if x is None:
                continue
            if kind == "device":
                import torch

                if isinstance(x, np.ndarray) or not getattr(x, "is_cuda", False) or x.dtype != torch.int32 \
                        or not x.is_contiguous() or x.dim() != 1 or x.numel() < n:
                    raise ValueError(f"{name}: a contiguous 1-D CUDA torch.int32 tensor of >= {n} elements (read as unsigned)")
            elif not isinstance(x, np.ndarray) or x.dtype != np.uint32 or not x.flags["C_CONTIGUOUS"] or x.ndim != 1 \
                    or x.size < n:
                raise ValueError(f"{name}: a C-contiguous 1-D numpy uint32 array of >= {n} elements")
        return (f.ctypes.data if f.size else None, None if r is None else r.ctypes.data, f.size, f, r,
                _size(image) // self.raw_block_size)

    def _u32_ptr(self, x):
        return None if x is None else self._index_ptr(x)

    def files_blocks(self, image, files, ranges=None, index=None, path_status=None, tree_index=None, tree_status=None,
                     file_flags=None, counts=None, write_back: bool = True, stream=None):
        """Device walk over a batch (ppfs_ecc_files_blocks_device); counts as in file_blocks, one record for the
        batch.  Never synchronises."""
        fp, rp, n, f, r, blocks = self._files_check("device", image, files, ranges, index, path_status, tree_index,
                                                    tree_status, file_flags)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_files_blocks_device(
            self._h, _ptr(image), blocks, fp, rp, n, self._u32_ptr(index), _ptr(path_status), self._u32_ptr(tree_index),
            _ptr(tree_status), self._u32_ptr(file_flags), None if d_counts is None else d_counts.data_ptr(),
            int(bool(write_back)), _stream_handle(stream)))
        return d_counts

    def files_blocks_host(self, image: np.ndarray, files, ranges=None, index=None, path_status=None, tree_index=None,
                          tree_status=None, file_flags=None, write_back: bool = True) -> "FileCounts":
        fp, rp, n, f, r, blocks = self._files_check("host", image, files, ranges, index, path_status, tree_index,
                                                    tree_status, file_flags)
        rec = _native.FileCounts()
        check(lib().ppfs_ecc_files_blocks_host(
            self._h, _ptr(image), blocks, fp, rp, n, self._u32_ptr(index), _ptr(path_status), self._u32_ptr(tree_index),
            _ptr(tree_status), self._u32_ptr(file_flags), byref(rec), int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, k)) for k in FILE_COUNT_FIELDS])

    def read_files(self, image, files, ranges, out, status=None, file_flags=None, counts=None, write_back: bool = True,
                   stream=None):
        """Device read of a batch (ppfs_ecc_read_files_device): out[slot.out_pos, + slot.bytes) = file f's range;
        status: one byte per file block touched, files back to back.  Never synchronises."""
        fp, rp, n, f, r, blocks = self._files_check("device", image, files, ranges, file_flags=file_flags, out=out,
                                                    status=status, read=True)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_read_files_device(
            self._h, _ptr(image), blocks, fp, rp, n, _ptr(out), 0 if out is None else _size(out), _ptr(status),
            self._u32_ptr(file_flags), None if d_counts is None else d_counts.data_ptr(), int(bool(write_back)),
            _stream_handle(stream)))
        return d_counts

    def read_files_host(self, image: np.ndarray, files, ranges, out: Optional[np.ndarray],
                        status: Optional[np.ndarray] = None, file_flags: Optional[np.ndarray] = None,
                        write_back: bool = True) -> "FileCounts":
        fp, rp, n, f, r, blocks = self._files_check("host", image, files, ranges, file_flags=file_flags, out=out,
                                                    status=status, read=True)
        rec = _native.FileCounts()
        check(lib().ppfs_ecc_read_files_host(
            self._h, _ptr(image), blocks, fp, rp, n, _ptr(out), 0 if out is None else _size(out), _ptr(status),
            self._u32_ptr(file_flags), byref(rec), int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, k)) for k in FILE_COUNT_FIELDS])

    # ---------------- write a file range from its inode (ppfs_ecc_write_file_*, ppfs_ecc_write_files_*) ----------------
    # FileIO::writeFile over an EXISTING range: offset + nbytes <= file_size, nothing grows and no inode is updated.
    # `data` holds the range's bytes (a batch: file f's at [slot.out_pos, + slot.bytes) of files_plan).  `written`: the
    # bytes that precede the first block with final status 5 or 9 (the range's bytes when none fails), one per file.
    # The device forms return (counts, written) as CUDA int64 tensors or None, the host forms (FileCounts, written).
    @staticmethod
    def _device_written(written, n: int):
        if written is None or written is False:
            return None
        import torch

        if written is True:
            return torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
        if not getattr(written, "is_cuda", False) or written.dtype != torch.int64 or not written.is_contiguous() \
                or written.dim() != 1 or written.numel() < n:
            raise ValueError(f"written: None, True or a contiguous 1-D CUDA int64 tensor of >= {n} elements")
        return written

    def _write_file_check(self, kind, data, image, file, offset, nbytes, status):
        f = self._file(file)
        if image is None:
            raise ValueError("image: required")
        if offset < 0 or nbytes < 0:
            raise ValueError("offset and nbytes must be >= 0")
        if nbytes and offset + nbytes > int(f["file_size"][0]):
            raise ValueError("the range runs past the file's end: a write does not grow the file")
        _, nblocks, _ = self.file_span(f, offset, nbytes)
        if nbytes and data is None:
            raise ValueError("data: required")
        _need("image", image, 0, kind)
        _need("data", data, nbytes, kind)
        _need("status", status, nblocks, kind)
        _ptr(image), _ptr(data), _ptr(status)  # contiguous uint8
        return f, _size(image) // self.raw_block_size, 0 if data is None else _size(data)

    def write_file(self, data, image, file, offset: int, nbytes: int, status=None, written=None, counts=None,
                   write_back: bool = True, stream=None):
        """Device file write (ppfs_ecc_write_file_device): data[0, nbytes) replaces the file range; status: one byte per
        file block touched; write_back applies to the index blocks.  Never synchronises."""
        f, blocks, in_bytes = self._write_file_check("device", data, image, file, offset, nbytes, status)
        d_counts, d_written = self._device_counts(counts), self._device_written(written, 1)
        check(lib().ppfs_ecc_write_file_device(
            self._h, _ptr(data), in_bytes, _ptr(image), blocks, f.ctypes.data, int(offset), int(nbytes), _ptr(status),
            None if d_written is None else d_written.data_ptr(), None if d_counts is None else d_counts.data_ptr(),
            int(bool(write_back)), _stream_handle(stream)))
        return d_counts, d_written

    def write_file_host(self, data: Optional[np.ndarray], image: np.ndarray, file, offset: int, nbytes: int,
                        status: Optional[np.ndarray] = None, write_back: bool = True):
        f, blocks, in_bytes = self._write_file_check("host", data, image, file, offset, nbytes, status)
        rec, written = _native.FileCounts(), ctypes.c_uint64(0)
        check(lib().ppfs_ecc_write_file_host(self._h, _ptr(data), in_bytes, _ptr(image), blocks, f.ctypes.data, int(offset),
                                             int(nbytes), _ptr(status), byref(written), byref(rec), int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, n)) for n in FILE_COUNT_FIELDS]), int(written.value)

    def _write_files_check(self, kind, data, image, files, ranges, status, file_flags):
        f, r = self._files(files, ranges)
        sizes = f["file_size"].astype(np.uint64)
        if r is not None and f.size:
            over = np.flatnonzero((r[:, 1] > 0) & ((r[:, 0] + r[:, 1] < r[:, 0]) | (r[:, 0] + r[:, 1] > sizes)))
            if over.size:
                raise ValueError(f"file {int(over[0])}: the range runs past the file's end: a write does not grow the file")
        args = self._files_check(kind, image, f, r, file_flags=file_flags, status=status)
        total = int(sizes.sum() if r is None else r[:, 1].sum())  # a write is never clamped
        if total and data is None:
            raise ValueError("data: required")
        _need("data", data, total, kind)
        _ptr(data)  # contiguous uint8
        return args

    def write_files(self, data, image, files, ranges=None, status=None, file_flags=None, written=None, counts=None,
                    write_back: bool = True, stream=None):
        """Device write of a batch (ppfs_ecc_write_files_device): data[slot.out_pos, + slot.bytes) replaces file f's
        range.  Two ranges of one inode record that share a file block are refused.  Never synchronises."""
        fp, rp, n, f, r, blocks = self._write_files_check("device", data, image, files, ranges, status, file_flags)
        d_counts, d_written = self._device_counts(counts), self._device_written(written, n)
        check(lib().ppfs_ecc_write_files_device(
            self._h, _ptr(data), 0 if data is None else _size(data), _ptr(image), blocks, fp, rp, n, _ptr(status),
            self._u32_ptr(file_flags), None if d_written is None else d_written.data_ptr(),
            None if d_counts is None else d_counts.data_ptr(), int(bool(write_back)), _stream_handle(stream)))
        return d_counts, d_written

    def write_files_host(self, data: Optional[np.ndarray], image: np.ndarray, files, ranges=None,
                         status: Optional[np.ndarray] = None, file_flags: Optional[np.ndarray] = None,
                         write_back: bool = True):
        """Host write of a batch; repeats are not refused: ranges apply in batch order."""
        fp, rp, n, f, r, blocks = self._write_files_check("host", data, image, files, ranges, status, file_flags)
        rec, written = _native.FileCounts(), np.zeros(max(n, 1), np.uint64)
        check(lib().ppfs_ecc_write_files_host(
            self._h, _ptr(data), 0 if data is None else _size(data), _ptr(image), blocks, fp, rp, n, _ptr(status),
            self._u32_ptr(file_flags), written.ctypes.data, byref(rec), int(bool(write_back))))
        return FileCounts(*[int(getattr(rec, k)) for k in FILE_COUNT_FIELDS]), written[:n]

    # ---------------- read inodes from the inode table (ppfs_ecc_inode_span, ppfs_ecc_read_inodes_*) ----------------
    # `table` is one INODE_TABLE_DTYPE record in host memory (table_block, bitmap_block, total_inodes, check_bitmap).
    # `numbers` names the inodes: a packed array of 32-bit numbers (device: a CUDA int32 tensor, read as unsigned; host:
    # a numpy uint32 array), or a uint8 buffer with `n` and `stride`, number j being the little-endian uint32 at byte
    # j * stride -- stride 128 over the payload of a directory as read_file(s) left it.  Outputs, each optional: files
    # (64 n bytes: FILE_DTYPE records), meta (24 n bytes: INODE_META_DTYPE), status (n), piece_status
    # (n * (1 + inode_max_pieces)), counts.
    @staticmethod
    def _inode_table(table) -> np.ndarray:
        t = np.ascontiguousarray(table)
        if t.dtype != _native.INODE_TABLE_DTYPE or t.size != 1:
            raise ValueError("table: one record of INODE_TABLE_DTYPE")
        return t.reshape(1)

    @property
    def inode_max_pieces(self) -> int:
        """K(ds): the most table pieces one inode has, 2 + 79 // data_size."""
        return 2 + 79 // self.data_size

    def inode_span(self, table, ino: int):
        """(block, offset, pieces) of inode `ino` in the inode table (ppfs_ecc_inode_span).  No GPU work."""
        t = self._inode_table(table)
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        if not 0 <= int(ino) <= 0xFFFFFFFF:
            raise ValueError("ino: an unsigned 32-bit number")
        check(lib().ppfs_ecc_inode_span(self._h, t.ctypes.data, int(ino), byref(a), byref(b), byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def _inodes_check(self, kind, image, table, numbers, n, stride, files, meta, status, piece_status):
        t = self._inode_table(table)
        if image is None:
            raise ValueError("image: required")
        if numbers is None:
            raise ValueError("numbers: required")
        _need("image", image, 0, kind)
        _ptr(image)
        packed = (numbers.dtype == np.uint32) if isinstance(numbers, np.ndarray) else (numbers.element_size() == 4)
        if kind == "device":
            if isinstance(numbers, np.ndarray) or not getattr(numbers, "is_cuda", False) or not numbers.is_contiguous():
                raise ValueError("numbers: a contiguous CUDA tensor (int32 numbers, or uint8 bytes with n and stride)")
            nbytes, addr = int(numbers.numel()) * numbers.element_size(), numbers.data_ptr()
        else:
            if not isinstance(numbers, np.ndarray) or not numbers.flags["C_CONTIGUOUS"]:
                raise ValueError("numbers: a C-contiguous numpy array (uint32 numbers, or uint8 bytes with n and stride)")
            nbytes, addr = int(numbers.nbytes), numbers.ctypes.data
        if packed:
            if n is None:
                n = nbytes // 4
            stride = 4 if stride is None else stride
        elif n is None or stride is None:
            raise ValueError("numbers: a byte buffer needs n and stride")
        n, stride = int(n), int(stride)
        if n < 0 or stride < 4:
            raise ValueError("n >= 0 and stride >= 4")
        if n and nbytes < (n - 1) * stride + 4:
            raise ValueError(f"numbers: {nbytes} bytes < {(n - 1) * stride + 4} needed")
        for name, x, per in (("files", files, 64), ("meta", meta, 24), ("status", status, 1),
                             ("piece_status", piece_status, 1 + self.inode_max_pieces)):
            if x is None:
                continue
            if kind == "device":
                if isinstance(x, np.ndarray) or not getattr(x, "is_cuda", False) or not x.is_contiguous() \
                        or x.numel() * x.element_size() < n * per:
                    raise ValueError(f"{name}: a contiguous CUDA tensor of >= {n * per} bytes")
            elif not isinstance(x, np.ndarray) or not x.flags["C_CONTIGUOUS"] or x.nbytes < n * per:
                raise ValueError(f"{name}: a C-contiguous numpy array of >= {n * per} bytes")
        return t, _size(image) // self.raw_block_size, addr if n else None, stride, n

    def read_inodes(self, image, table, numbers, n=None, stride=None, files=None, meta=None, status=None, piece_status=None,
                    counts=None, write_back: bool = True, stream=None):
        """Device read of a batch of inodes (ppfs_ecc_read_inodes_device).  counts: None, True (a fresh CUDA int64
        tensor of the eight words of INODE_COUNT_FIELDS) or such a tensor.  Never synchronises."""
        t, blocks, addr, stride, n = self._inodes_check("device", image, table, numbers, n, stride, files, meta, status,
                                                        piece_status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_read_inodes_device(
            self._h, _ptr(image), blocks, t.ctypes.data, addr, stride, n, self._u32_ptr(files), self._u32_ptr(meta),
            self._u32_ptr(status), self._u32_ptr(piece_status), None if d_counts is None else d_counts.data_ptr(),
            int(bool(write_back)), _stream_handle(stream)))
        return d_counts

    def read_inodes_host(self, image: np.ndarray, table, numbers, n=None, stride=None, files=None, meta=None, status=None,
                         piece_status=None, write_back: bool = True) -> "InodeCounts":
        t, blocks, addr, stride, n = self._inodes_check("host", image, table, numbers, n, stride, files, meta, status,
                                                        piece_status)
        rec = _native.InodeCounts()
        check(lib().ppfs_ecc_read_inodes_host(
            self._h, _ptr(image), blocks, t.ctypes.data, addr, stride, n, self._u32_ptr(files), self._u32_ptr(meta),
            self._u32_ptr(status), self._u32_ptr(piece_status), byref(rec), int(bool(write_back))))
        return InodeCounts(*[int(getattr(rec, k)) for k in INODE_COUNT_FIELDS])

    # ---------------- write inodes into the inode table (ppfs_ecc_write_inodes_*) ----------------
    # InodeManager::update over a batch: the reads' arguments with `files` (64 n bytes) and `meta` (24 n bytes) as
    # required inputs; status, piece_status and counts are the outputs.
    def write_inodes(self, image, table, numbers, files, meta, n=None, stride=None, status=None, piece_status=None,
                     counts=None, write_back: bool = True, stream=None):
        """Device write of a batch of inodes (ppfs_ecc_write_inodes_device): inode j's 81 bytes are meta[j]'s two
        times, the 64 bytes of files[j] and meta[j]'s type.  Several inodes of one table block and repeated numbers
        are the norm: the result is the per-inode loop's in batch order.  counts as for read_inodes.  Never
        synchronises."""
        if files is None or meta is None:
            raise ValueError("files and meta: required")
        t, blocks, addr, stride, n = self._inodes_check("device", image, table, numbers, n, stride, files, meta, status,
                                                        piece_status)
        d_counts = self._device_counts(counts)
        check(lib().ppfs_ecc_write_inodes_device(
            self._h, _ptr(image), blocks, t.ctypes.data, addr, stride, n, self._u32_ptr(files), self._u32_ptr(meta),
            self._u32_ptr(status), self._u32_ptr(piece_status), None if d_counts is None else d_counts.data_ptr(),
            int(bool(write_back)), _stream_handle(stream)))
        return d_counts

    def write_inodes_host(self, image: np.ndarray, table, numbers, files, meta, n=None, stride=None, status=None,
                          piece_status=None, write_back: bool = True) -> "InodeCounts":
        if files is None or meta is None:
            raise ValueError("files and meta: required")
        t, blocks, addr, stride, n = self._inodes_check("host", image, table, numbers, n, stride, files, meta, status,
                                                        piece_status)
        rec = _native.InodeCounts()
        check(lib().ppfs_ecc_write_inodes_host(
            self._h, _ptr(image), blocks, t.ctypes.data, addr, stride, n, self._u32_ptr(files), self._u32_ptr(meta),
            self._u32_ptr(status), self._u32_ptr(piece_status), byref(rec), int(bool(write_back))))
        return InodeCounts(*[int(getattr(rec, k)) for k in INODE_COUNT_FIELDS])

    # ---------------- look up names in directories (ppfs_ecc_lookup_*) ----------------
    # DirectoryManager::getInodeByName (mode 0) or the search of removeEntry (mode 1) over a batch: `dirs` is a
    # FILE_DTYPE array in host memory, `queries` a LOOKUP_QUERY_DTYPE array in host memory, `names` the nq 128-byte name
    # records (lookup_names packs them).  Every directory is read once and whole: `entries` and `block_status`, sized by
    # lookup_plan, are the call's working memory and hold the entries and final block statuses afterwards as read_files
    # leaves them, so `entries` is a ready `numbers` source at stride 128 for read_inodes.
    @staticmethod
    def lookup_names(names) -> np.ndarray:
        """An (n, 128) uint8 array of name records out of bytes / str names of at most 123 bytes."""
        out = np.zeros((len(names), _native.LOOKUP_NAME_BYTES), dtype=np.uint8)
        for i, name in enumerate(names):
            b = name.encode() if isinstance(name, str) else bytes(name)
            if len(b) > 123 or 0 in b:
                raise ValueError("a name holds at most 123 bytes and no NUL")
            out[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        return out

    def lookup_plan(self, dirs):
        """(slots, totals) of the directories' entries (ppfs_ecc_lookup_plan): files_plan over the ranges
        (0, 128 * entries).  totals["bytes"] sizes the entries buffer, totals["blocks"] the block statuses.  No GPU work."""
        f, _ = self._files(dirs, None)
        slots, totals = np.zeros(f.size, _native.FILES_SLOT_DTYPE), np.zeros(1, _native.FILES_TOTALS_DTYPE)
        check(lib().ppfs_ecc_lookup_plan(self._h, f.ctypes.data if f.size else None, f.size,
                                         slots.ctypes.data if f.size else None, totals.ctypes.data))
        return slots, totals[0]

    def _lookup_check(self, kind, image, dirs, queries, names, mode, entries, block_status, dir_flags):
        f, _ = self._files(dirs, None)
        q = np.ascontiguousarray(queries)
        if q.dtype != _native.LOOKUP_QUERY_DTYPE or q.ndim > 1:
            raise ValueError("queries: a 1-D array of LOOKUP_QUERY_DTYPE records")
        q = q.reshape(-1)
        if mode not in (0, 1):
            raise ValueError("mode: 0 (name) or 1 (inode number)")
        if image is None:
            raise ValueError("image: required")
        _, totals = self.lookup_plan(f)
        _need("image", image, 0, kind)
        if mode == 0:
            if names is None and q.size:
                raise ValueError("names: required in name mode")
            _need("names", names, q.size * _native.LOOKUP_NAME_BYTES, kind)
        _need("entries", entries, int(totals["bytes"]), kind)
        _need("block_status", block_status, int(totals["blocks"]), kind)
        _ptr(image), _ptr(names), _ptr(entries), _ptr(block_status)  # contiguous uint8
        if dir_flags is not None:
            if kind == "device":
                import torch

                if isinstance(dir_flags, np.ndarray) or not getattr(dir_flags, "is_cuda", False) or dir_flags.dtype != torch.int32 \
                        or not dir_flags.is_contiguous() or dir_flags.numel() < f.size:
                    raise ValueError(f"dir_flags: a contiguous CUDA torch.int32 tensor of >= {f.size} elements")
            elif not isinstance(dir_flags, np.ndarray) or dir_flags.dtype != np.uint32 or not dir_flags.flags["C_CONTIGUOUS"] \
                    or dir_flags.size < f.size:
                raise ValueError(f"dir_flags: a C-contiguous numpy uint32 array of >= {f.size} elements")
        return f, q, _size(image) // self.raw_block_size

    def lookup(self, image, dirs, queries, names, mode: int, entries, block_status, hits, dir_flags=None, counts=None,
               file_counts=None, write_back: bool = True, stream=None):
        """Device lookup (ppfs_ecc_lookup_device).  names: a CUDA uint8 tensor of 128 bytes per query (mode 1: None);
        entries, block_status: CUDA uint8 tensors, required; hits: a contiguous CUDA int32 tensor of 4 words per query
        (LOOKUP_HIT_DTYPE once on the host).  counts / file_counts: None, True or a CUDA int64 tensor of 8 words
        (LOOKUP_COUNT_FIELDS / FILE_COUNT_FIELDS).  Returns (counts, file_counts).  Never synchronises."""
        f, q, blocks = self._lookup_check("device", image, dirs, queries, names, mode, entries, block_status, dir_flags)
        if entries is None or block_status is None:
            raise ValueError("entries and block_status: the call's working memory, required in the device form")
        import torch

        if hits is None or isinstance(hits, np.ndarray) or not getattr(hits, "is_cuda", False) or hits.dtype != torch.int32 \
                or not hits.is_contiguous() or hits.numel() < 4 * q.size:
            raise ValueError(f"hits: a contiguous CUDA torch.int32 tensor of >= {4 * q.size} elements")
        d_counts, d_file_counts = self._device_counts(counts), self._device_counts(file_counts)
        check(lib().ppfs_ecc_lookup_device(
            self._h, _ptr(image), blocks, f.ctypes.data if f.size else None, f.size, q.ctypes.data if q.size else None,
            _ptr(names), q.size, int(mode), _ptr(entries), _size(entries), _ptr(block_status), self._u32_ptr(dir_flags),
            hits.data_ptr(), None if d_counts is None else d_counts.data_ptr(),
            None if d_file_counts is None else d_file_counts.data_ptr(), int(bool(write_back)), _stream_handle(stream)))
        return d_counts, d_file_counts

    def lookup_host(self, image: np.ndarray, dirs, queries, names, mode: int = 0, entries: Optional[np.ndarray] = None,
                    block_status: Optional[np.ndarray] = None, dir_flags: Optional[np.ndarray] = None,
                    write_back: bool = True):
        """Host lookup (ppfs_ecc_lookup_host): (hits, LookupCounts, FileCounts), hits a LOOKUP_HIT_DTYPE array.
        entries and block_status may be None: the call then uses buffers of its own."""
        f, q, blocks = self._lookup_check("host", image, dirs, queries, names, mode, entries, block_status, dir_flags)
        hits = np.zeros(q.size, _native.LOOKUP_HIT_DTYPE)
        rec, frec = _native.LookupCounts(), _native.FileCounts()
        check(lib().ppfs_ecc_lookup_host(
            self._h, _ptr(image), blocks, f.ctypes.data if f.size else None, f.size, q.ctypes.data if q.size else None,
            _ptr(names), q.size, int(mode), _ptr(entries), 0 if entries is None else _size(entries), _ptr(block_status),
            self._u32_ptr(dir_flags), hits.ctypes.data if q.size else None, byref(rec), byref(frec), int(bool(write_back))))
        return (hits, LookupCounts(*[int(getattr(rec, k)) for k in LOOKUP_COUNT_FIELDS]),
                FileCounts(*[int(getattr(frec, k)) for k in FILE_COUNT_FIELDS]))


# ppfs_ecc_scrub_counts: the host forms return it as this tuple, the device forms as a CUDA int64 tensor
# in the same field order (ScrubCounts(*tensor.tolist()) after synchronising)
SCRUB_COUNT_FIELDS = ("ok", "corrected", "failed", "out_of_range", "not_allocated", "bitmap_ok", "bitmap_corrected",
                      "bitmap_failed")
ScrubCounts = collections.namedtuple("ScrubCounts", SCRUB_COUNT_FIELDS)
# ppfs_ecc_file_counts, likewise
FILE_COUNT_FIELDS = ("ok", "corrected", "failed", "out_of_range", "index_ok", "index_corrected", "index_failed",
                     "index_out_of_range")
FileCounts = collections.namedtuple("FileCounts", FILE_COUNT_FIELDS)
FILE_DTYPE = _native.FILE_DTYPE
# ppfs_ecc_inode_counts, likewise: the five categories, then the three reserved words
INODE_COUNT_FIELDS = ("ok", "corrected", "failed", "out_of_range", "not_allocated", "reserved0", "reserved1", "reserved2")
InodeCounts = collections.namedtuple("InodeCounts", INODE_COUNT_FIELDS)
INODE_TABLE_DTYPE = _native.INODE_TABLE_DTYPE
INODE_META_DTYPE = _native.INODE_META_DTYPE
# ppfs_ecc_lookup_counts, likewise: the four categories, then the four reserved words
LOOKUP_COUNT_FIELDS = ("found", "not_found", "failed", "out_of_range", "reserved0", "reserved1", "reserved2", "reserved3")
LookupCounts = collections.namedtuple("LookupCounts", LOOKUP_COUNT_FIELDS)
LOOKUP_QUERY_DTYPE = _native.LOOKUP_QUERY_DTYPE
LOOKUP_HIT_DTYPE = _native.LOOKUP_HIT_DTYPE


class EccGroup:
    """Multi-GPU host path (include/ppfs_ecc.h ppfs_ecc_group_*): one context per
    listed device (a device may repeat); the *_host calls shard a batch into contiguous block
    ranges, one host thread per context, with no data exchanged between devices."""

    def __init__(self, ecc_type: int, block_size: int, rs_correctable_bytes: int = 3,
                 crc_polynomial_explicit: int = 0, devices=(0,)):
        p = EccParams(int(ecc_type), int(block_size), int(rs_correctable_bytes), 0, int(crc_polynomial_explicit))
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = c_void_p()
        check(lib().ppfs_ecc_group_create(byref(p), devs, len(devices), byref(h)))
        self._h = h
        self.devices = tuple(int(d) for d in devices)
        c0 = lib().ppfs_ecc_group_ctx(h, 0)
        self.raw_block_size = int(lib().ppfs_ecc_raw_block_size(c0))
        self.data_size = int(lib().ppfs_ecc_data_size(c0))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ppfs_ecc_group_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, n, data=None, raw=None, status=None, spill=None) -> None:
        _need("data", data, n * self.data_size, "host")
        _need("raw", raw, n * self.raw_block_size, "host")
        _need("status", status, n, "host")
        _need("spill", spill, n * (256 - min(self.raw_block_size, 255)), "host")

    def encode_host(self, data: np.ndarray, raw: np.ndarray) -> None:
        n = _host_blocks(data, self.data_size, "data")
        self._check(n, data, raw)
        check(lib().ppfs_ecc_group_encode_host(self._h, _ptr(data), _ptr(raw), n))

    def decode_host(self, raw: np.ndarray, data: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None,
                    write_back: bool = True, spill: Optional[np.ndarray] = None) -> None:
        n = _host_blocks(raw, self.raw_block_size, "raw")
        self._check(n, data, raw, status, spill)
        check(lib().ppfs_ecc_group_decode_host(self._h, _ptr(raw), _ptr(data), _ptr(status), n,
                                               int(bool(write_back)), _ptr(spill)))

    def write_host(self, data: np.ndarray, raw: np.ndarray, status: Optional[np.ndarray] = None) -> None:
        n = _host_blocks(data, self.data_size, "data")
        self._check(n, data, raw, status)
        check(lib().ppfs_ecc_group_write_host(self._h, _ptr(data), _ptr(raw), _ptr(status), n))


class pinned:
    """Page-lock numpy arrays for the duration of a `with` block (ppfs_ecc_host_register): the
    *_host calls then DMA them directly instead of copying through staging buffers."""

    def __init__(self, *arrays: np.ndarray):
        self._arrays = [a for a in arrays if a is not None and a.nbytes]

    def __enter__(self):
        done = []
        try:
            for a in self._arrays:
                check(lib().ppfs_ecc_host_register(_ptr(a), a.nbytes))
                done.append(a)
        except Exception:
            for a in done:
                lib().ppfs_ecc_host_unregister(_ptr(a))
            raise
        return self

    def __exit__(self, *exc):
        # every array is released even when one release fails; the first failure is raised after
        rcs = [lib().ppfs_ecc_host_unregister(_ptr(a)) for a in self._arrays]
        for rc in rcs:
            check(rc)
        return False


def vote3_host(a: np.ndarray, b: np.ndarray, c: np.ndarray, rec_bytes: Optional[int] = None, device: int = 0):
    """2-of-3 bitwise majority of replicated records (SuperBlockManager::_performBitVoting,
    super_block_manager.cpp:133-165) on the GPU.  Returns (voted bytes, per-record damage bits:
    bit k = copy k+1 differs from the majority)."""
    a, b, c = (np.ascontiguousarray(x, dtype=np.uint8).reshape(-1) for x in (a, b, c))
    if not (a.size == b.size == c.size):
        raise ValueError("vote3: copies differ in size")
    rb = int(rec_bytes) if rec_bytes is not None else a.size
    if rb < 0 or (rb == 0 and a.size) or (rb and a.size % rb):
        raise ValueError("vote3: the copies must hold a whole number of records")
    nrec = a.size // rb if rb else 0
    out = np.empty_like(a)
    dmg = np.zeros(nrec, dtype=np.uint32)
    check(lib().ppfs_vote3_host(int(device), _ptr(a), _ptr(b), _ptr(c), _ptr(out), rb, nrec, dmg.ctypes.data))
    return out, dmg


def vote3(a, b, c, out, rec_bytes: int, damaged=None, stream=None) -> None:
    """Device-resident vote3 over torch uint8 tensors; damaged: int32 tensor of nrec (or None)."""
    if rec_bytes <= 0:
        raise ValueError("vote3: rec_bytes must be > 0")
    nrec = a.numel() // rec_bytes
    nbytes = nrec * rec_bytes
    for name, x in (("b", b), ("c", c), ("out", out)):
        _need(name, x, nbytes, "device")
    _need("a", a, nbytes, "device")
    if damaged is not None:
        if damaged.element_size() != 4 or not damaged.is_contiguous() or damaged.numel() < nrec:
            raise ValueError("vote3: damaged must be a contiguous 4-byte tensor of >= nrec elements")
        if not damaged.is_cuda:
            raise ValueError("vote3: damaged must be a CUDA tensor")
    dptr = None if damaged is None else damaged.data_ptr()
    check(lib().ppfs_vote3_device(_ptr(a), _ptr(b), _ptr(c), _ptr(out), rec_bytes, nrec, dptr,
                                  _stream_handle(stream)))


def device_copy(dst, src, nbytes: Optional[int] = None, stream=None) -> None:
    """dst[:nbytes] = src[:nbytes] on the device (torch uint8 tensors): the full-grid copy kernel
    bench.py times as the HBM ceiling next to the roofline (not part of the reference interface)."""
    n = int(src.numel() if nbytes is None else nbytes)
    if n > dst.numel() or n > src.numel():
        raise ValueError("device_copy: nbytes exceeds a buffer")
    check(lib().ppfs_copy_device(_ptr(dst), _ptr(src), n, _stream_handle(stream)))


def inject_bytes(raw, stride: int, pos, val, nblocks: Optional[int] = None, xor: bool = False, stream=None) -> None:
    """Corrupt one byte per block of a device raw image (torch uint8 tensors): block b's byte
    pos[b] becomes val[b] (or byte ^ val[b] with xor=True); pos[b] >= stride skips the block.
    bench.py's fault injection (not part of the reference interface; the reference's bit flipper,
    usage_simulator/simulation/src/bit_flipper.cpp, is a simulator and out of scope)."""
    nb = int(pos.numel() if nblocks is None else nblocks)
    for name, t in (("raw", raw), ("pos", pos), ("val", val)):
        if not t.is_cuda or t.element_size() != 1 or not t.is_contiguous():
            raise ValueError(f"inject_bytes: {name} must be a contiguous CUDA uint8 tensor")
    if stride <= 0 or nb > pos.numel() or nb > val.numel() or nb * stride > raw.numel():
        raise ValueError("inject_bytes: a buffer is shorter than nblocks implies")
    check(lib().ppfs_inject_device(_ptr(raw), stride, nb, _ptr(pos), _ptr(val), 1 if xor else 0,
                                   _stream_handle(stream)))


def crc_implicit_to_explicit(p: int) -> int:
    """CrcPolynomial::MsgImplicit (crc_polynomial.cpp:41-54) -> explicit form."""
    return int(lib().ppfs_ecc_crc_implicit_to_explicit(ctypes.c_uint64(p)))


__all__ = ["EccEngine", "ScrubCounts", "SCRUB_COUNT_FIELDS", "FileCounts", "FILE_COUNT_FIELDS", "FILE_DTYPE", "InodeCounts", "INODE_COUNT_FIELDS", "INODE_TABLE_DTYPE", "INODE_META_DTYPE", "LookupCounts", "LOOKUP_COUNT_FIELDS", "LOOKUP_QUERY_DTYPE", "LOOKUP_HIT_DTYPE", "crc_implicit_to_explicit", "device_copy", "inject_bytes", "pinned", "vote3", "vote3_host", "_native"]
