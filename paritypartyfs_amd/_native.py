"""ctypes binding of the C ABI in include/ppfs_ecc.h (libppfs_ecc.so, built in-tree).

The library is the product path: it holds the HIP kernels for gfx950.  Loading fails loudly
when it is missing -- there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_longlong, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PPFS_ECC_LIB: an alternative build of the same library (ablation runs, tools/)
LIB_PATH = os.environ.get("PPFS_ECC_LIB") or os.path.join(_HERE, "_lib", "libppfs_ecc.so")

# ECCType (lib/blockdevice/include/ppfs/blockdevice/ecc_type.hpp:8-14)
ECC_NONE, ECC_CRC, ECC_HAMMING, ECC_PARITY, ECC_REED_SOLOMON = 0, 1, 2, 3, 4

STATUS_OK, STATUS_CORRECTED, STATUS_CORRECTION_ERROR = 0, 1, 5
STATUS_OUT_OF_BOUNDS = 9  # a block-list entry past the image (FsError::Disk_OutOfBounds)
STATUS_NOT_ALLOCATED = 255  # scrub_allocated: the block's bit is clear, the block was not read
STATUS_NOT_FOUND = 2  # lookup: the query's loop ran to its end without a match (PPFS_ECC_NOT_FOUND)

# every symbol include/ppfs_ecc.h declares
EXPORTED_SYMBOLS = (
    "ppfs_ecc_crc_implicit_to_explicit",
    "ppfs_ecc_create",
    "ppfs_ecc_destroy",
    "ppfs_ecc_raw_block_size",
    "ppfs_ecc_data_size",
    "ppfs_ecc_kernel_name",
    "ppfs_ecc_stream_kernel_name",
    "ppfs_ecc_time_next_launch",
    "ppfs_ecc_encode_device",
    "ppfs_ecc_decode_device",
    "ppfs_ecc_write_device",
    "ppfs_ecc_encode_host",
    "ppfs_ecc_decode_host",
    "ppfs_ecc_write_host",
    "ppfs_ecc_host_chunk_blocks",
    "ppfs_ecc_list_kernel_name",
    "ppfs_ecc_list_encode_kernel_name",
    "ppfs_ecc_decode_list_device",
    "ppfs_ecc_encode_list_device",
    "ppfs_ecc_write_list_device",
    "ppfs_ecc_decode_list_host",
    "ppfs_ecc_encode_list_host",
    "ppfs_ecc_write_list_host",
    "ppfs_ecc_read_extents_device",
    "ppfs_ecc_write_extents_device",
    "ppfs_ecc_read_extents_host",
    "ppfs_ecc_write_extents_host",
    "ppfs_ecc_scrub_host",
    "ppfs_ecc_scrub_device",
    "ppfs_ecc_scrub_list_device",
    "ppfs_ecc_scrub_list_host",
    "ppfs_ecc_scrub_allocated_device",
    "ppfs_ecc_scrub_allocated_host",
    "ppfs_ecc_file_span",
    "ppfs_ecc_file_tree_blocks",
    "ppfs_ecc_file_blocks_device",
    "ppfs_ecc_file_blocks_host",
    "ppfs_ecc_read_file_device",
    "ppfs_ecc_read_file_host",
    "ppfs_ecc_files_plan",
    "ppfs_ecc_files_blocks_device",
    "ppfs_ecc_files_blocks_host",
    "ppfs_ecc_read_files_device",
    "ppfs_ecc_read_files_host",
    "ppfs_ecc_write_file_device",
    "ppfs_ecc_write_file_host",
    "ppfs_ecc_write_files_device",
    "ppfs_ecc_write_files_host",
    "ppfs_ecc_inode_span",
    "ppfs_ecc_read_inodes_device",
    "ppfs_ecc_read_inodes_host",
    "ppfs_ecc_write_inodes_device",
    "ppfs_ecc_write_inodes_host",
    "ppfs_ecc_lookup_plan",
    "ppfs_ecc_lookup_device",
    "ppfs_ecc_lookup_host",
    "ppfs_vote3_device",
    "ppfs_vote3_host",
    "ppfs_copy_device",
    "ppfs_inject_device",
    "ppfs_ecc_host_register",
    "ppfs_ecc_host_unregister",
    "ppfs_ecc_host_registered",
    "ppfs_ecc_group_create",
    "ppfs_ecc_group_destroy",
    "ppfs_ecc_group_size",
    "ppfs_ecc_group_ctx",
    "ppfs_ecc_group_encode_host",
    "ppfs_ecc_group_decode_host",
    "ppfs_ecc_group_write_host",
    "ppfs_ecc_last_error",
    "ppfs_ecc_debug_faults",
    "ppfs_ecc_debug_selftest",
    "ppfs_ecc_debug_dma_rejects",
    "ppfs_ecc_debug_dma_selftest",
)


# ppfs_ecc_extent: one (block, offset, length) entry of the byte-extent calls and where its bytes lie
# in the packed caller buffer
EXTENT_DTYPE = np.dtype([("pos", "<u8"), ("block", "<u4"), ("offset", "<u2"), ("length", "<u2")])

# ppfs_ecc_file: the 64 bytes of an Inode that the read-only file walk reads
FILE_DTYPE = np.dtype([("direct", "<u4", (12,)), ("indirect", "<u4"), ("doubly_indirect", "<u4"),
                       ("trebly_indirect", "<u4"), ("file_size", "<u4")])

# ppfs_ecc_files_slot: where one file of a batch lies in the batch's arrays (88 bytes), and
# ppfs_ecc_files_totals: the batch's sizes (48 bytes)
FILES_SLOT_DTYPE = np.dtype([("first_block", "<u8"), ("blocks", "<u8"), ("bytes", "<u8"), ("block_pos", "<u8"),
                             ("out_pos", "<u8"), ("tree_pos", "<u8", (3,)), ("tree_n", "<u8", (3,))])
FILES_TOTALS_DTYPE = np.dtype([("blocks", "<u8"), ("bytes", "<u8"), ("tree_level", "<u8", (3,)), ("tree_blocks", "<u8")])

# ppfs_ecc_inode_table: the SuperBlock fields InodeManager reads (16 bytes), and ppfs_ecc_inode_meta: what an Inode
# holds besides its ppfs_ecc_file record (24 bytes)
INODE_TABLE_DTYPE = np.dtype([("table_block", "<u4"), ("bitmap_block", "<u4"), ("total_inodes", "<u4"), ("check_bitmap", "<u4")])
INODE_META_DTYPE = np.dtype([("time_creation", "<u8"), ("time_modified", "<u8"), ("type", "u1"), ("pad", "u1", (7,))])
INODE_PIECE = 16384  # PPFS_ECC_INODE_PIECE: inodes per piece of a device call

# ppfs_ecc_lookup_query: one (directory, key) of a lookup (8 bytes), and ppfs_ecc_lookup_hit: its answer (16 bytes);
# a name key is a 128-byte record of its own (LOOKUP_NAME_BYTES), NUL-terminated within its first 124 bytes
LOOKUP_QUERY_DTYPE = np.dtype([("dir", "<u4"), ("key", "<u4")])
LOOKUP_HIT_DTYPE = np.dtype([("inode", "<u4"), ("entry", "<u4"), ("status", "<u4"), ("reserved", "<u4")])
LOOKUP_NAME_BYTES = 128
LOOKUP_NONE = 0xFFFFFFFF  # inode and entry of a hit whose status is not 0


class EccParams(ctypes.Structure):
    _fields_ = [
        ("ecc_type", c_uint32),
        ("block_size", c_uint32),
        ("rs_correctable_bytes", c_uint32),
        ("reserved", c_uint32),
        ("crc_polynomial", c_uint64),
    ]


class ScrubCounts(ctypes.Structure):
    """ppfs_ecc_scrub_counts: what a list / allocated scrub found (64 bytes, overwritten by each call)."""
    _fields_ = [(n, c_uint64) for n in ("ok", "corrected", "failed", "out_of_range", "not_allocated", "bitmap_ok",
                                        "bitmap_corrected", "bitmap_failed")]


class FileCounts(ctypes.Structure):
    """ppfs_ecc_file_counts: what a file walk / file read found (64 bytes, overwritten by each call)."""
    _fields_ = [(n, c_uint64) for n in ("ok", "corrected", "failed", "out_of_range", "index_ok", "index_corrected",
                                        "index_failed", "index_out_of_range")]


class InodeCounts(ctypes.Structure):
    """ppfs_ecc_inode_counts: the statuses of a batch of inode reads (64 bytes, overwritten by each call)."""
    _fields_ = [(n, c_uint64) for n in ("ok", "corrected", "failed", "out_of_range", "not_allocated", "reserved0",
                                        "reserved1", "reserved2")]


class LookupCounts(ctypes.Structure):
    """ppfs_ecc_lookup_counts: the statuses of a batch of lookups (64 bytes, overwritten by each call)."""
    _fields_ = [(n, c_uint64) for n in ("found", "not_found", "failed", "out_of_range", "reserved0", "reserved1",
                                        "reserved2", "reserved3")]


class NativeLibraryMissing(RuntimeError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    """Load libppfs_ecc.so (raises NativeLibraryMissing if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build it with `make -C paritypartyfs_amd/csrc` "
            "(or __graft_entry__.build()); the HIP engine has no CPU fallback")
    # torch bundles its own libamdhip64; with both runtimes in one process torch's has to
    # initialise first (measured: the other order leaves torch with "No HIP GPUs are available")
    try:
        import torch

        torch.cuda.is_available()
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    u8p = POINTER(c_uint8)
    L.ppfs_ecc_debug_faults.restype = c_longlong
    L.ppfs_ecc_debug_faults.argtypes = []
    L.ppfs_ecc_debug_selftest.restype = c_longlong
    L.ppfs_ecc_debug_selftest.argtypes = []
    L.ppfs_ecc_debug_dma_rejects.restype = c_longlong
    L.ppfs_ecc_debug_dma_rejects.argtypes = []
    L.ppfs_ecc_debug_dma_selftest.restype = c_longlong
    L.ppfs_ecc_debug_dma_selftest.argtypes = []
    L.ppfs_ecc_host_registered.restype = c_longlong
    L.ppfs_ecc_host_registered.argtypes = [POINTER(c_size_t)]
    L.ppfs_ecc_time_next_launch.restype = c_int
    L.ppfs_ecc_time_next_launch.argtypes = [c_void_p, c_void_p]
    L.ppfs_ecc_stream_kernel_name.restype = c_char_p
    L.ppfs_ecc_stream_kernel_name.argtypes = [c_void_p, c_void_p]
    L.ppfs_ecc_crc_implicit_to_explicit.restype = c_uint64
    L.ppfs_ecc_crc_implicit_to_explicit.argtypes = [c_uint64]
    L.ppfs_ecc_create.restype = c_int
    L.ppfs_ecc_create.argtypes = [POINTER(EccParams), c_int, POINTER(c_void_p)]
    L.ppfs_ecc_destroy.restype = None
    L.ppfs_ecc_destroy.argtypes = [c_void_p]
    L.ppfs_ecc_raw_block_size.restype = c_size_t
    L.ppfs_ecc_raw_block_size.argtypes = [c_void_p]
    L.ppfs_ecc_data_size.restype = c_size_t
    L.ppfs_ecc_data_size.argtypes = [c_void_p]
    L.ppfs_ecc_kernel_name.restype = c_char_p
    L.ppfs_ecc_kernel_name.argtypes = [c_void_p]
    L.ppfs_ecc_encode_device.restype = c_int
    L.ppfs_ecc_encode_device.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    L.ppfs_ecc_decode_device.restype = c_int
    L.ppfs_ecc_decode_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p,
                                         c_void_p]
    L.ppfs_ecc_write_device.restype = c_int
    L.ppfs_ecc_write_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    L.ppfs_ecc_host_chunk_blocks.restype = c_size_t
    L.ppfs_ecc_host_chunk_blocks.argtypes = [c_void_p]
    L.ppfs_ecc_encode_host.restype = c_int
    L.ppfs_ecc_encode_host.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    L.ppfs_ecc_decode_host.restype = c_int
    L.ppfs_ecc_decode_host.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
    L.ppfs_ecc_write_host.restype = c_int
    L.ppfs_ecc_write_host.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]
    L.ppfs_ecc_list_kernel_name.restype = c_char_p
    L.ppfs_ecc_list_kernel_name.argtypes = [c_void_p]
    L.ppfs_ecc_list_encode_kernel_name.restype = c_char_p
    L.ppfs_ecc_list_encode_kernel_name.argtypes = [c_void_p]
    # block lists: (ctx, image, image_blocks, index, nblocks, data, status, write_back, spill[, stream])
    L.ppfs_ecc_decode_list_device.restype = c_int
    L.ppfs_ecc_decode_list_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_int,
                                              c_void_p, c_void_p]
    L.ppfs_ecc_encode_list_device.restype = c_int
    L.ppfs_ecc_encode_list_device.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]
    L.ppfs_ecc_write_list_device.restype = c_int
    L.ppfs_ecc_write_list_device.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t,
                                             c_void_p]
    L.ppfs_ecc_decode_list_host.restype = c_int
    L.ppfs_ecc_decode_list_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_int,
                                            c_void_p]
    L.ppfs_ecc_encode_list_host.restype = c_int
    L.ppfs_ecc_encode_list_host.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]
    L.ppfs_ecc_write_list_host.restype = c_int
    L.ppfs_ecc_write_list_host.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t]
    # byte extents: read (ctx, image, image_blocks, ext, n, out, out_bytes, status, write_back[, stream]),
    # write (ctx, in, in_bytes, image, image_blocks, ext, n, status[, stream])
    L.ppfs_ecc_read_extents_device.restype = c_int
    L.ppfs_ecc_read_extents_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                               c_void_p, c_int, c_void_p]
    L.ppfs_ecc_write_extents_device.restype = c_int
    L.ppfs_ecc_write_extents_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                                c_void_p, c_void_p]
    L.ppfs_ecc_read_extents_host.restype = c_int
    L.ppfs_ecc_read_extents_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                             c_void_p, c_int]
    L.ppfs_ecc_write_extents_host.restype = c_int
    L.ppfs_ecc_write_extents_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                              c_void_p]
    L.ppfs_ecc_scrub_host.restype = c_int
    L.ppfs_ecc_scrub_host.argtypes = [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, POINTER(c_size_t)]
    L.ppfs_ecc_scrub_device.restype = c_int
    L.ppfs_ecc_scrub_device.argtypes = [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]
    # list scrub: (ctx, image, image_blocks, index, nblocks, status, counts[, stream]); allocated scrub:
    # (ctx, image, image_blocks, bitmap_block, first_block, nbits, status, bitmap_status, counts[, stream])
    L.ppfs_ecc_scrub_list_device.restype = c_int
    L.ppfs_ecc_scrub_list_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
    L.ppfs_ecc_scrub_list_host.restype = c_int
    L.ppfs_ecc_scrub_list_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]
    L.ppfs_ecc_scrub_allocated_device.restype = c_int
    L.ppfs_ecc_scrub_allocated_device.argtypes = [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_size_t, c_void_p,
                                                  c_void_p, c_void_p, c_void_p]
    L.ppfs_ecc_scrub_allocated_host.restype = c_int
    L.ppfs_ecc_scrub_allocated_host.argtypes = [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_size_t, c_void_p,
                                                c_void_p, c_void_p]
    # file walk: span (ctx, file, offset, nbytes, &first, &nblocks, &clamped); tree_blocks (ctx, file, first, nblocks);
    # blocks (ctx, image, image_blocks, file, first, nblocks, index, path_status, tree_index, tree_status, counts,
    # write_back[, stream]); read (ctx, image, image_blocks, file, offset, nbytes, out, out_bytes, status, counts,
    # write_back[, stream])
    L.ppfs_ecc_file_span.restype = c_int
    L.ppfs_ecc_file_span.argtypes = [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_uint64), POINTER(c_uint64),
                                     POINTER(c_uint64)]
    L.ppfs_ecc_file_tree_blocks.restype = c_longlong
    L.ppfs_ecc_file_tree_blocks.argtypes = [c_void_p, c_void_p, c_uint64, c_uint64]
    L.ppfs_ecc_file_blocks_device.restype = c_int
    L.ppfs_ecc_file_blocks_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_file_blocks_host.restype = c_int
    L.ppfs_ecc_file_blocks_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_int]
    L.ppfs_ecc_read_file_device.restype = c_int
    L.ppfs_ecc_read_file_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64, c_void_p, c_size_t,
                                            c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_read_file_host.restype = c_int
    L.ppfs_ecc_read_file_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64, c_void_p, c_size_t,
                                          c_void_p, c_void_p, c_int]
    # batches of files: plan (ctx, files, ranges, nfiles, slots, totals); blocks (ctx, image, image_blocks, files, ranges,
    # nfiles, index, path_status, tree_index, tree_status, file_flags, counts, write_back[, stream]); read (ctx, image,
    # image_blocks, files, ranges, nfiles, out, out_bytes, status, file_flags, counts, write_back[, stream])
    L.ppfs_ecc_files_plan.restype = c_int
    L.ppfs_ecc_files_plan.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    L.ppfs_ecc_files_blocks_device.restype = c_int
    L.ppfs_ecc_files_blocks_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_files_blocks_host.restype = c_int
    L.ppfs_ecc_files_blocks_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    L.ppfs_ecc_read_files_device.restype = c_int
    L.ppfs_ecc_read_files_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                             c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_read_files_host.restype = c_int
    L.ppfs_ecc_read_files_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                           c_void_p, c_void_p, c_void_p, c_int]
    # file writes: (ctx, in, in_bytes, image, image_blocks, file, offset, nbytes, status, written, counts, write_back
    # [, stream]) and (ctx, in, in_bytes, image, image_blocks, files, ranges, nfiles, status, file_flags, written, counts,
    # write_back[, stream])
    L.ppfs_ecc_write_file_device.restype = c_int
    L.ppfs_ecc_write_file_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64,
                                             c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_write_file_host.restype = c_int
    L.ppfs_ecc_write_file_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_uint64, c_uint64,
                                           c_void_p, c_void_p, c_void_p, c_int]
    L.ppfs_ecc_write_files_device.restype = c_int
    L.ppfs_ecc_write_files_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_write_files_host.restype = c_int
    L.ppfs_ecc_write_files_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    # inode reads: span (ctx, table, ino, block, offset, pieces); read (ctx, image, image_blocks, table, ino, ino_stride,
    # n, files, meta, status, piece_status, counts, write_back[, stream])
    L.ppfs_ecc_inode_span.restype = c_int
    L.ppfs_ecc_inode_span.argtypes = [c_void_p, c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]
    L.ppfs_ecc_read_inodes_device.restype = c_int
    L.ppfs_ecc_read_inodes_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_read_inodes_host.restype = c_int
    L.ppfs_ecc_read_inodes_host.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_int]
    # inode writes: the reads' arguments, files and meta inputs
    L.ppfs_ecc_write_inodes_device.restype = c_int
    L.ppfs_ecc_write_inodes_device.argtypes = list(L.ppfs_ecc_read_inodes_device.argtypes)
    L.ppfs_ecc_write_inodes_host.restype = c_int
    L.ppfs_ecc_write_inodes_host.argtypes = list(L.ppfs_ecc_read_inodes_host.argtypes)
    # lookups: plan (ctx, dirs, ndirs, slots, totals); lookup (ctx, image, image_blocks, dirs, ndirs, queries, names, nq,
    # mode, entries, entries_bytes, block_status, dir_flags, hits, counts, file_counts, write_back[, stream])
    L.ppfs_ecc_lookup_plan.restype = c_int
    L.ppfs_ecc_lookup_plan.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    L.ppfs_ecc_lookup_device.restype = c_int
    L.ppfs_ecc_lookup_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_int,
                                         c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_ecc_lookup_host.restype = c_int
    L.ppfs_ecc_lookup_host.argtypes = list(L.ppfs_ecc_lookup_device.argtypes[:-1])
    L.ppfs_vote3_device.restype = c_int
    L.ppfs_vote3_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]
    L.ppfs_copy_device.restype = c_int
    L.ppfs_copy_device.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    L.ppfs_inject_device.restype = c_int
    L.ppfs_inject_device.argtypes = [c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_int, c_void_p]
    L.ppfs_vote3_host.restype = c_int
    L.ppfs_vote3_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]
    L.ppfs_ecc_host_register.restype = c_int
    L.ppfs_ecc_host_register.argtypes = [c_void_p, c_size_t]
    L.ppfs_ecc_host_unregister.restype = c_int
    L.ppfs_ecc_host_unregister.argtypes = [c_void_p]
    L.ppfs_ecc_group_create.restype = c_int
    L.ppfs_ecc_group_create.argtypes = [POINTER(EccParams), POINTER(c_int), c_int, POINTER(c_void_p)]
    L.ppfs_ecc_group_destroy.restype = None
    L.ppfs_ecc_group_destroy.argtypes = [c_void_p]
    L.ppfs_ecc_group_size.restype = c_int
    L.ppfs_ecc_group_size.argtypes = [c_void_p]
    L.ppfs_ecc_group_ctx.restype = c_void_p
    L.ppfs_ecc_group_ctx.argtypes = [c_void_p, c_int]
    L.ppfs_ecc_group_encode_host.restype = c_int
    L.ppfs_ecc_group_encode_host.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    L.ppfs_ecc_group_decode_host.restype = c_int
    L.ppfs_ecc_group_decode_host.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
    L.ppfs_ecc_group_write_host.restype = c_int
    L.ppfs_ecc_group_write_host.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]
    L.ppfs_ecc_last_error.restype = c_char_p
    L.ppfs_ecc_last_error.argtypes = []
    _ = u8p
    _lib = L
    return L


class EccError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"ppfs_ecc error {code}: {what}")
        self.code = code


def check(rc: int) -> None:
    if rc != 0:
        raise EccError(rc, lib().ppfs_ecc_last_error().decode(errors="replace"))


def host_registered() -> tuple[int, int] | None:
    """(ranges, bytes) still registered through ppfs_ecc_host_register; None if the library is not
    loaded yet (nothing can have been registered through it then)."""
    if _lib is None:
        return None
    b = c_size_t(0)
    n = int(_lib.ppfs_ecc_host_registered(ctypes.byref(b)))
    return n, int(b.value)


def debug_dma_rejects() -> int | None:
    """Copies a PPFS_ECC_DEBUG build refused (an end not page-locked / device memory over its whole
    range); None for a normal build or when the library is not loaded yet."""
    if _lib is None:
        return None
    v = int(_lib.ppfs_ecc_debug_dma_rejects())
    return None if v < 0 else v


def debug_faults() -> int | None:
    """Out-of-bounds global accesses detected so far by a PPFS_ECC_DEBUG build of the library
    (csrc/dbg.hpp); None when the loaded library is a normal build or is not loaded yet."""
    if _lib is None:
        return None
    v = int(_lib.ppfs_ecc_debug_faults())
    if v == -1:
        return None
    if v < 0:
        raise RuntimeError(f"ppfs_ecc_debug_faults failed ({v})")
    return v
