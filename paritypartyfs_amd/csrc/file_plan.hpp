#pragma once
// file_plan.hpp -- the arithmetic of the file walk (files_path.cpp, files_walk.hip): how the 64
// bytes of an inode that describe its index-block tree (inode.hpp:18-41) and a range of file blocks
// become the image blocks to read, as FileIO's BlockIndexIterator finds them (file_io.cpp:186-463,
// should_resize == false).  Plain arithmetic for host and device alike, so the kernels, the host forms,
// the adapters and tests/cpp/test_file_plan.cpp (a plain g++ program under the address sanitizer) decide
// identically.
//
// The tree.  ds = dataSize(), I = ipb = ds / 4 entries per index block (little-endian uint32 at payload
// bytes [4 slot, 4 slot + 4); payload bytes past 4 I are ignored).  File block j lies in one of four
// SEGMENTS:
//   0  j < 12                        direct[j]
//   1  s = j - 12 < I                entry s of block `indirect`
//   2  s = j - 12 - I < I^2          entry s / I of `doubly_indirect` names a leaf, entry s % I of the leaf
//   3  s = j - 12 - I - I^2 < I^3    entry s / I^2 of `trebly_indirect` names a mid block, entry
//                                    (s / I) % I of the mid block a leaf, entry s % I of the leaf
// A walk over the file blocks [j0, j1) reads each index block above them once.  They are taken in three
// LEVELS, each one list decode, in this fixed order (also the order of tree_index / tree_status):
//   A  the roots visited, in the order indirect, doubly_indirect, trebly_indirect
//   B  the doubly tree's leaves ascending, then the trebly tree's mid blocks ascending
//   C  the trebly tree's leaves ascending
// An entry's pointer comes from its PARENT: the inode record (taken as sixteen dwords: direct[0..11],
// indirect, doubly_indirect, trebly_indirect, file_size) or slot `slot` of entry `parent_k` of the level
// above.  In the scratch of a call the levels start on 16-entry boundaries (slot_base), so that each
// level's payload and status pointers keep the list decode's 16-byte rule; in the caller's arrays they lie
// back to back (entry_base).
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace fileplan {

constexpr uint32_t DIRECT = 12;              // direct pointers of an inode
constexpr uint32_t NO_BLOCK = 0xFFFFFFFFu;   // the pointer of an entry whose path failed: in no image
constexpr uint8_t STATUS_FAILED = 5, STATUS_OUT = 9;
// file blocks per piece of a device read: bounds the per-block scratch (index 4, path status 1, extent
// 16, read status 1 = 22 bytes per block, 704 KiB a piece)
constexpr uint64_t PIECE_BLOCKS = 1ull << 15;
enum Level : int { LEVEL_INODE = -1, LEVEL_A = 0, LEVEL_B = 1, LEVEL_C = 2, LEVEL_DATA = 3 };
// the inode record's dwords that hold the three roots
constexpr uint32_t DW_INDIRECT = 12, DW_DOUBLY = 13, DW_TREBLY = 14;

PPFS_HD inline uint64_t ipb_of(uint64_t ds) { return ds / 4u; }
PPFS_HD inline uint64_t capacity_ipb(uint64_t I) { return DIRECT + I + I * I + I * I * I; }
// file blocks the tree can hold (64-bit: I <= 16,383 for a 16-bit block size)
PPFS_HD inline uint64_t capacity(uint64_t ds) { return capacity_ipb(ipb_of(ds)); }
// blocks a file of file_size bytes occupies; 0 for a codec without payload
PPFS_HD inline uint64_t occupied(uint64_t file_size, uint64_t ds) { return ds ? (file_size + ds - 1u) / ds : 0u; }

// Where file block j lies: its segment (4: past the tree), depth = index blocks above it (= segment) and
// the slot taken at each of them, outermost first; slot[0] of segment 0 is the direct pointer's number.
struct Path {
    uint32_t segment, depth;
    uint64_t slot[3];
};
PPFS_HD inline Path path_of(uint64_t j, uint64_t I)
{
    Path p { 4u, 0u, { 0, 0, 0 } };
    if (j < DIRECT) {
        p.segment = 0;
        p.slot[0] = j;
        return p;
    }
    uint64_t s = j - DIRECT;
    if (s < I) {
        p.segment = p.depth = 1;
        p.slot[0] = s;
        return p;
    }
    s -= I;
    if (s < I * I) {
        p.segment = p.depth = 2;
        p.slot[0] = s / I;
        p.slot[1] = s % I;
        return p;
    }
    s -= I * I;
    if (s < I * I * I) {
        p.segment = p.depth = 3;
        p.slot[0] = s / (I * I);
        p.slot[1] = (s / I) % I;
        p.slot[2] = s % I;
    }
    return p;
}

// readFile(offset, nbytes) of a file of file_size bytes (file_io.cpp:12-44): the first file block, the
// number of blocks and the bytes delivered.  ok == false: offset >= file_size with nbytes > 0 (or a codec
// without payload).  nbytes == 0 is an empty, valid range.
struct Span {
    uint64_t first, count, bytes;
    bool ok;
};
PPFS_HD inline Span span(uint64_t file_size, uint64_t ds, uint64_t offset, uint64_t nbytes)
{
    if (nbytes == 0)
        return Span { 0, 0, 0, true };
    if (ds == 0 || offset >= file_size)
        return Span { 0, 0, 0, false };
    const uint64_t left = file_size - offset, bytes = nbytes < left ? nbytes : left;
    return Span { offset / ds, (offset % ds + bytes + ds - 1u) / ds, bytes, true };
}

// Block i of such a read (i = 0 for the first): where its bytes lie in the packed buffer, from which
// payload byte and how many -- extent_plan.hpp file_extents without the scan.  off0 = offset % ds.
struct Extent {
    uint64_t pos;
    uint32_t offset, length;
};
PPFS_HD inline Extent extent_of(uint64_t i, uint64_t off0, uint64_t bytes, uint64_t ds)
{
    const uint64_t pos = i == 0 ? 0u : i * ds - off0, off = i == 0 ? off0 : 0u;
    const uint64_t left = pos < bytes ? bytes - pos : 0u, len = ds - off < left ? ds - off : left;
    return Extent { pos, (uint32_t)off, (uint32_t)len };
}

// The index blocks of a walk over the file blocks [j0, j1), j1 <= capacity_ipb(I)
struct Tree {
    uint64_t j0, j1, I;
    uint64_t S1, S2;           // first file block of segments 2 and 3 (segment 1 starts at DIRECT)
    uint32_t a_ind, a_dbl, a_trb; // 1 when the walk visits that root
    uint64_t d0, d1;           // the walk's part of segment 2, relative to S1 (d0 == d1: none)
    uint64_t t0, t1;           // the walk's part of segment 3, relative to S2
    uint64_t nA, nBd, nBt, nB, nC; // entries per level; nB = nBd leaves of the doubly tree + nBt mid blocks
};
PPFS_HD inline uint64_t clampu(uint64_t v, uint64_t lo, uint64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
PPFS_HD inline Tree tree_of(uint64_t j0, uint64_t count, uint64_t I)
{
    Tree t {};
    t.j0 = j0;
    t.j1 = j0 + count;
    t.I = I;
    t.S1 = DIRECT + I;
    t.S2 = t.S1 + I * I;
    const uint64_t S3 = t.S2 + I * I * I;
    if (count == 0 || I == 0)
        return t;
    t.a_ind = clampu(t.j0, DIRECT, t.S1) < clampu(t.j1, DIRECT, t.S1);
    t.d0 = clampu(t.j0, t.S1, t.S2) - t.S1;
    t.d1 = clampu(t.j1, t.S1, t.S2) - t.S1;
    t.t0 = clampu(t.j0, t.S2, S3) - t.S2;
    t.t1 = clampu(t.j1, t.S2, S3) - t.S2;
    t.a_dbl = t.d0 < t.d1;
    t.a_trb = t.t0 < t.t1;
    if (!t.a_dbl)
        t.d0 = t.d1 = 0;
    if (!t.a_trb)
        t.t0 = t.t1 = 0;
    t.nA = t.a_ind + t.a_dbl + t.a_trb;
    t.nBd = t.a_dbl ? (t.d1 - 1u) / I - t.d0 / I + 1u : 0u;
    t.nBt = t.a_trb ? (t.t1 - 1u) / (I * I) - t.t0 / (I * I) + 1u : 0u;
    t.nB = t.nBd + t.nBt;
    t.nC = t.a_trb ? (t.t1 - 1u) / I - t.t0 / I + 1u : 0u;
    return t;
}
PPFS_HD inline uint64_t level_count(const Tree& t, int level)
{
    return level == LEVEL_A ? t.nA : level == LEVEL_B ? t.nB : level == LEVEL_C ? t.nC : t.j1 - t.j0;
}
PPFS_HD inline uint64_t tree_blocks(const Tree& t) { return t.nA + t.nB + t.nC; }
// where a level starts in the caller's tree_index / tree_status ...
PPFS_HD inline uint64_t entry_base(const Tree& t, int level) { return level == LEVEL_A ? 0u : level == LEVEL_B ? t.nA : t.nA + t.nB; }
// ... and in a call's scratch, where every level starts on a 16-entry boundary
PPFS_HD inline uint64_t round16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
PPFS_HD inline uint64_t slot_base(const Tree& t, int level)
{
    return level == LEVEL_A ? 0u : level == LEVEL_B ? 16u : 16u + round16(t.nB);
}
PPFS_HD inline uint64_t tree_slots(const Tree& t) { return 16u + round16(t.nB) + t.nC; }

// Entry k of a level (LEVEL_DATA: file block j0 + k): where its pointer stands.  level == LEVEL_INODE:
// dword `slot` of the inode record; else slot `slot` of entry parent_k of that level.
struct Ref {
    int level;
    uint64_t parent_k;
    uint32_t slot;
};
PPFS_HD inline Ref ref_of(const Tree& t, int level, uint64_t k)
{
    const uint64_t I = t.I;
    switch (level) {
    case LEVEL_A: {
        // the k-th visited root in the order indirect, doubly, trebly
        uint32_t dw = DW_INDIRECT;
        uint64_t seen = 0;
        if (t.a_ind && seen++ == k)
            dw = DW_INDIRECT;
        else if (t.a_dbl && seen++ == k)
            dw = DW_DOUBLY;
        else
            dw = DW_TREBLY;
        return Ref { LEVEL_INODE, 0, dw };
    }
    case LEVEL_B:
        if (k < t.nBd)
            return Ref { LEVEL_A, t.a_ind, (uint32_t)(t.d0 / I + k) };
        return Ref { LEVEL_A, (uint64_t)t.a_ind + t.a_dbl, (uint32_t)(t.t0 / (I * I) + (k - t.nBd)) };
    case LEVEL_C: {
        const uint64_t leaf = t.t0 / I + k;
        return Ref { LEVEL_B, t.nBd + (leaf / I - t.t0 / (I * I)), (uint32_t)(leaf % I) };
    }
    default: {
        const uint64_t j = t.j0 + k;
        if (j < DIRECT)
            return Ref { LEVEL_INODE, 0, (uint32_t)j };
        if (j < t.S1)
            return Ref { LEVEL_A, 0, (uint32_t)(j - DIRECT) };
        if (j < t.S2) {
            const uint64_t s = j - t.S1;
            return Ref { LEVEL_B, s / I - t.d0 / I, (uint32_t)(s % I) };
        }
        const uint64_t s = j - t.S2;
        return Ref { LEVEL_C, s / I - t.t0 / I, (uint32_t)(s % I) };
    }
    }
}

// the first requested file block under tree entry k of a level: the entry is read immediately before
// that block, outer levels first (the order of the reference's reads and of its correction log)
PPFS_HD inline uint64_t first_under(const Tree& t, int level, uint64_t k)
{
    const uint64_t I = t.I;
    uint64_t at = t.j0;
    if (level == LEVEL_A) {
        const uint32_t dw = ref_of(t, LEVEL_A, k).slot;
        at = dw == DW_INDIRECT ? DIRECT : dw == DW_DOUBLY ? t.S1 : t.S2;
    } else if (level == LEVEL_B) {
        at = k < t.nBd ? t.S1 + (t.d0 / I + k) * I : t.S2 + (t.t0 / (I * I) + (k - t.nBd)) * I * I;
    } else if (level == LEVEL_C) {
        at = t.S2 + (t.t0 / I + k) * I;
    }
    return at > t.j0 ? at : t.j0;
}

// What an expansion reads -- inode(dw): dword dw of the inode record; status(slot) / inherited(slot):
// the decode status and the inherited path status of the tree entry in scratch slot `slot`;
// payload_byte(at): byte `at` of the payload scratch (slot * ds + byte).
//
// Entry k of a level: its pointer and the status it inherits.  A parent whose own path failed, or whose
// decode gave 5 (payload undefined) or 9 (no such block), hands that status down and the pointer becomes
// NO_BLOCK; a corrected parent (1) hands down nothing.
struct Expanded {
    uint32_t pointer;
    uint8_t inherited;
};
// expand_at: the same with the scratch positions of this file's levels A, B, C given (base_a, base_b,
// base_c) -- a batch of files keeps every level of all its files in one merged list (files_plan.hpp);
// expand: one file, whose levels start at slot_base.
template <class Src>
PPFS_HD inline Expanded expand_at(const Tree& t, int level, uint64_t k, uint64_t ds, const Src& src, uint64_t base_a,
    uint64_t base_b, uint64_t base_c)
{
    const Ref r = ref_of(t, level, k);
    if (r.level == LEVEL_INODE)
        return Expanded { src.inode(r.slot), 0 };
    const uint64_t p = (r.level == LEVEL_A ? base_a : r.level == LEVEL_B ? base_b : base_c) + r.parent_k;
    uint32_t ps = src.inherited(p);
    if (!ps)
        ps = src.status(p);
    if (ps == STATUS_FAILED || ps == STATUS_OUT)
        return Expanded { NO_BLOCK, (uint8_t)ps };
    const uint64_t at = p * ds + 4u * r.slot;
    const uint32_t v = src.payload_byte(at) | src.payload_byte(at + 1u) << 8 | src.payload_byte(at + 2u) << 16
        | src.payload_byte(at + 3u) << 24;
    return Expanded { v, 0 };
}
template <class Src>
PPFS_HD inline Expanded expand(const Tree& t, int level, uint64_t k, uint64_t ds, const Src& src)
{
    return expand_at(t, level, k, ds, src, slot_base(t, LEVEL_A), slot_base(t, LEVEL_B), slot_base(t, LEVEL_C));
}

// where a status lands in either half of ppfs_ecc_file_counts (four 64-bit words: ok, corrected, failed,
// out_of_range); -1 for a value that is none of the four
PPFS_HD inline int count_slot(uint32_t st) { return st == 0u ? 0 : st == 1u ? 1 : st == 5u ? 2 : st == 9u ? 3 : -1; }
constexpr int SLOT_FILE = 0, SLOT_INDEX = 4;

} // namespace fileplan
} // namespace ppfs
