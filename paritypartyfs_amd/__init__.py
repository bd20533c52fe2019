"""paritypartyfs_amd -- MI355X-native per-block ECC engine behind PPFS's block-device layer.

Product path: paritypartyfs_amd/csrc (HIP kernels for gfx950 + the C ABI of include/ppfs_ecc.h),
loaded from the in-tree libppfs_ecc.so.  Python pieces:
  - ecc.EccEngine            batch encode/decode/write/scrub on HBM tensors or host arrays, contiguous
                             ranges, block lists or byte extents (block, offset, length); scrub of a
                             block list or of the blocks an on-disk allocation bitmap marks; a file read
                             from the 64 bytes of its inode (file_blocks / read_file: the index-block tree
                             is resolved on the GPU), a batch of files (files_blocks / read_files), and the
                             in-place write of a file range or a batch of them (write_file / write_files);
                             a batch of inodes read out of the inode table (read_inodes) or written into it
                             (write_inodes); a batch of (directory, name) or (directory, inode number) lookups
                             (lookup)
  - ecc.EccGroup             the host calls sharded over several GPUs (one thread per device)
  - ecc.vote3 / vote3_host   2-of-3 bitwise voting of replicated records (superblock copies)
  - block_device.*           IBlockDevice mirror (ReedSolomon/Crc/Hamming/Parity/Raw devices)
"""
from ._native import (ECC_CRC, ECC_HAMMING, ECC_NONE, ECC_PARITY, ECC_REED_SOLOMON, STATUS_CORRECTED,
                      STATUS_CORRECTION_ERROR, STATUS_NOT_ALLOCATED, STATUS_NOT_FOUND, STATUS_OK, STATUS_OUT_OF_BOUNDS, FILE_DTYPE, FILES_SLOT_DTYPE, FILES_TOTALS_DTYPE,
                      INODE_META_DTYPE, INODE_TABLE_DTYPE, LOOKUP_HIT_DTYPE, LOOKUP_QUERY_DTYPE, NativeLibraryMissing)
from .ecc import EccEngine, EccGroup, FileCounts, InodeCounts, LookupCounts, ScrubCounts, crc_implicit_to_explicit, device_copy, inject_bytes, pinned, vote3, vote3_host

__all__ = [
    "EccEngine", "EccGroup", "ScrubCounts", "FileCounts", "FILE_DTYPE", "FILES_SLOT_DTYPE", "FILES_TOTALS_DTYPE", "InodeCounts", "INODE_TABLE_DTYPE", "INODE_META_DTYPE", "LookupCounts", "LOOKUP_QUERY_DTYPE", "LOOKUP_HIT_DTYPE", "crc_implicit_to_explicit", "device_copy", "inject_bytes", "pinned", "vote3", "vote3_host", "NativeLibraryMissing",
    "ECC_NONE", "ECC_CRC", "ECC_HAMMING", "ECC_PARITY", "ECC_REED_SOLOMON",
    "STATUS_OK", "STATUS_CORRECTED", "STATUS_CORRECTION_ERROR", "STATUS_OUT_OF_BOUNDS", "STATUS_NOT_ALLOCATED", "STATUS_NOT_FOUND",
]
