#pragma once
// inode_plan.hpp -- the arithmetic and the per-inode rule of the inode reads and writes (inode_path.cpp,
// inode_walk.hip): where the reference's InodeManager::get and update (lib/inode_manager/src/inode_manager.cpp:127-159)
// find inode i, and what they decide about it, as plain numbers.  For host and device alike, so the kernels, the host
// forms and tests/cpp/test_inode_plan.cpp (the same plan against a literal restatement of the reference's loops, under
// the sanitizers) decide identically.
//
// The packed Inode (inode.hpp:18-41) is INODE_BYTES = 81 bytes: time_creation [0, 8), time_modified [8, 16),
// direct[12] [16, 64), indirect 64, doubly_indirect 68, trebly_indirect 72, file_size 76, type 80.  ppfs_ecc_file is
// bytes [16, 80) of it.
// Inode i lies at table byte 81 i (_getInodeLocation, :11-18): block table_block + 81 i / ds, offset 81 i % ds, in
// 64-bit arithmetic.  _readInode (:56-89) reads the 81 bytes as a plain cut at block boundaries, since readBlock
// clamps to ds - offset (rs_block_device.cpp:28-48): pieces(i) = (81 i % ds + 80) / ds + 1 of them, at most
// K(ds) = 2 + 79 / ds.
// Bit i of the inode bitmap is byte i / 8 of the bitmap's payload stream under mask 0x80 >> (i % 8)
// (Bitmap::_getByteLocation / getBit, bitmap.cpp:8-14, 87-101; alloc_plan.hpp has the same convention): block
// bitmap_block + (i / 8) / ds, offset (i / 8) % ds.  In this bitmap a SET bit means FREE (InodeManager::create /
// remove / format), and get answers InodeManager_NotFound for it.
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace inodeplan {

constexpr uint32_t INODE_BYTES = 81, FILE_OFF = 16, FILE_BYTES = 64, TYPE_OFF = 80;
constexpr uint32_t NO_BLOCK = 0xFFFFFFFFu; // names no block: the extent calls treat it as invalid
constexpr uint32_t ST_OK = 0, ST_CORRECTED = 1, ST_FAILED = 5, ST_OUT = 9, ST_NOT_ALLOCATED = 255;
constexpr uint32_t ST_UNUSED = 255; // a piece_status slot that is unused or was never read
constexpr uint64_t PIECE_INODES = 16384; // PPFS_ECC_INODE_PIECE

// K(ds): the most pieces an inode can have.  ds > 0.
PPFS_HD inline uint32_t max_pieces(uint64_t ds) { return 2u + (uint32_t)(79u / ds); }
PPFS_HD inline uint32_t pieces(uint64_t ino, uint64_t ds) { return (uint32_t)(((uint64_t)INODE_BYTES * ino % ds + 80u) / ds) + 1u; }

// Inodes per piece of a device call: PIECE_INODES at K = 2, fewer where an inode has more pieces, so that a piece's
// K extents per inode stay within 2 * PIECE_INODES = one piece of the file walk's extent stream.
PPFS_HD inline uint64_t piece_inodes(uint64_t ds) { return 2u * PIECE_INODES / max_pieces(ds); }

// Piece k < pieces(ino, ds): `length` bytes at `offset` of block `block`, which are bytes [pos, pos + length) of
// the 81.  The block is a 64-bit number; one at or past NO_BLOCK names no block of any image.
struct Piece {
    uint64_t block;
    uint32_t offset, length, pos;
};
PPFS_HD inline Piece piece(uint32_t table_block, uint64_t ino, uint32_t k, uint64_t ds)
{
    const uint64_t byte = (uint64_t)INODE_BYTES * ino, b0 = (uint64_t)table_block + byte / ds, o0 = byte % ds;
    const uint64_t first = ds - o0 < INODE_BYTES ? ds - o0 : INODE_BYTES; // bytes of piece 0
    if (k == 0)
        return Piece { b0, (uint32_t)o0, (uint32_t)first, 0u };
    const uint64_t pos = first + (uint64_t)(k - 1u) * ds, left = INODE_BYTES - pos;
    return Piece { b0 + k, 0u, (uint32_t)(left < ds ? left : ds), (uint32_t)pos };
}

// the byte of the bitmap that holds bit `ino`, and the bit's mask in it
struct BitByte {
    uint64_t block;
    uint32_t offset, mask;
};
PPFS_HD inline BitByte bitmap_byte(uint32_t bitmap_block, uint64_t ino, uint64_t ds)
{
    const uint64_t byte = ino / 8u;
    return BitByte { (uint64_t)bitmap_block + byte / ds, (uint32_t)(byte % ds), 0x80u >> (uint32_t)(ino % 8u) };
}

// ---- the status rule of one inode, in the per-inode loop's order of evaluation ----
// Step 1 and 2, what getBit and the test of its answer decide: 0 = the table is read, else the inode's status.
//   ino >= total_inodes                      9 (Bitmap_IndexOutOfRange), with or without check_bitmap
//   check_bitmap: the byte's read status     5 or 9 as it stands
//                 a set bit                  255, free (InodeManager_NotFound)
PPFS_HD inline uint32_t bitmap_verdict(uint64_t ino, uint64_t total_inodes, bool check_bitmap, uint32_t read_status, uint32_t byte,
    uint32_t mask)
{
    if (ino >= total_inodes)
        return ST_OUT;
    if (!check_bitmap)
        return 0u;
    if (read_status == ST_FAILED || read_status == ST_OUT)
        return read_status;
    return (byte & mask) ? ST_NOT_ALLOCATED : 0u;
}
// Steps 3 and 4 for an inode whose verdict is 0: the first piece in order with status 5 or 9 gives that status (a
// table block at or past the image reads as 9); otherwise 1 if the bitmap byte or any piece reported 1, else 0.
// piece_status(k): the read status of piece k < npieces.  bitmap_status: the byte's, 0 when it was not read.
template <class PieceStatus>
PPFS_HD inline uint32_t table_status(uint32_t bitmap_status, uint32_t npieces, PieceStatus piece_status)
{
    uint32_t corrected = bitmap_status == ST_CORRECTED ? 1u : 0u;
    for (uint32_t k = 0; k < npieces; ++k) {
        const uint32_t s = piece_status(k);
        if (s == ST_FAILED || s == ST_OUT)
            return s;
        corrected |= s == ST_CORRECTED ? 1u : 0u;
    }
    return corrected ? ST_CORRECTED : ST_OK;
}

// ppfs_ecc_inode_table by value, for host and device
struct Table {
    uint32_t table_block, bitmap_block, total_inodes, check_bitmap;
};
// What steps 1 and 2 decide for inode `ino` from its bitmap byte and the byte's read status: the verdict, whether the
// bit was read at all, and the status piece_status slot 0 reports (ST_UNUSED when it was not).  A byte that was not
// delivered is not looked at.
struct BitmapStep {
    uint32_t verdict, bitmap_status;
    bool bit_read;
};
PPFS_HD inline BitmapStep bitmap_step(const Table& t, uint32_t ino, uint32_t byte, uint32_t read_status)
{
    const bool bit_read = ino < t.total_inodes && t.check_bitmap;
    const bool seen = bit_read && (read_status == ST_OK || read_status == ST_CORRECTED);
    return BitmapStep { bitmap_verdict(ino, t.total_inodes, t.check_bitmap != 0, read_status, seen ? byte : 0u, 0x80u >> (ino % 8u)),
        bit_read ? read_status : ST_UNUSED, bit_read };
}
// The epilogue of one inode: its final status, and into `row` (may be null) its 1 + K bytes of piece_status: the
// bitmap status, then the statuses of its pieces, ST_UNUSED behind the last one and throughout when the table was
// not read.  piece_status(k): the status of piece k < pieces(ino, ds).
template <class PieceStatus>
PPFS_HD inline uint32_t inode_status(const BitmapStep& b, uint32_t ino, uint64_t ds, uint32_t K, PieceStatus piece_status, uint8_t* row)
{
    const uint32_t np = b.verdict == 0u ? pieces(ino, ds) : 0u;
    const uint32_t st = b.verdict ? b.verdict : table_status(b.bit_read ? b.bitmap_status : 0u, np, piece_status);
    if (row) {
        row[0] = (uint8_t)b.bitmap_status;
        for (uint32_t k = 0; k < K; ++k)
            row[1u + k] = (uint8_t)(k < np ? piece_status(k) : ST_UNUSED);
    }
    return st;
}

// What slot k < K of an inode does: it TAKES PART when the verdict is 0, k < pieces(ino, ds) and its block is below
// NO_BLOCK, and then `length` bytes at `offset` of `block` are bytes [pos, pos + length) of the 81
struct Slot {
    bool takes_part;
    uint32_t block, offset, length, pos;
};
PPFS_HD inline Slot slot_of(uint32_t table_block, uint32_t ino, uint32_t k, uint32_t verdict, uint64_t ds)
{
    Slot s { false, NO_BLOCK, 0, 0, 0 };
    if (verdict != 0u || k >= pieces(ino, ds))
        return s;
    const Piece p = piece(table_block, ino, k, ds);
    if (p.block >= NO_BLOCK)
        return s;
    return Slot { true, (uint32_t)p.block, p.offset, p.length, p.pos };
}
// the read's extent of slot s of inode j of a piece (Extent: ppfs_ecc_extent's fields in its order): the slot's bytes
// land at 81 j + pos of the rows; a slot that does not take part gives the invalid extent
template <class Extent>
PPFS_HD inline Extent slot_extent(const Slot& s, uint64_t j)
{
    return s.takes_part ? Extent { (uint64_t)INODE_BYTES * j + s.pos, s.block, (uint16_t)s.offset, (uint16_t)s.length }
                        : Extent { 0, NO_BLOCK, 0, 0 };
}

// where a status lands in ppfs_ecc_inode_counts taken as eight 64-bit words: ok, corrected, failed, out_of_range,
// not_allocated; -1 for any other value
PPFS_HD inline int count_slot(uint32_t st) { return st == 0u ? 0 : st == 1u ? 1 : st == 5u ? 2 : st == 9u ? 3 : st == 255u ? 4 : -1; }
constexpr int SLOT_NOT_ALLOCATED = 4;

// little-endian fields out of a byte source `at(i)`, i < 81
template <class At>
PPFS_HD inline uint32_t le32(At at, uint32_t i)
{
    return (uint32_t)at(i) | (uint32_t)at(i + 1u) << 8 | (uint32_t)at(i + 2u) << 16 | (uint32_t)at(i + 3u) << 24;
}
template <class At>
PPFS_HD inline uint64_t le64(At at, uint32_t i)
{
    return (uint64_t)le32(at, i) | (uint64_t)le32(at, i + 4u) << 32;
}

} // namespace inodeplan
} // namespace ppfs
