#pragma once
// list_store.hpp -- the store plan of the list encode's emission (rs_wg_list.hpp): which bytes of a
// tile row go to which addresses of the image, and with which store.  The counterpart of
// list_fetch.hpp: plain arithmetic for host and device alike, so the kernel's emission and
// tests/cpp/test_list_store.cpp (the same plan over a heap image, under the address sanitizer)
// decide identically.
//
// Row r of a 64-row tile is the codeword of list entry r and goes to d = image + index[r] * 255, at
// any byte alignment (the image's base included).  With a = d mod 16 and h = (16 - a) mod 16:
//   head   codeword bytes [0, h)            d + [0, h)          up to the first 16-byte boundary
//   full   window j = 0..14: bytes [h + 16 j, h + 16 j + 16), one aligned 16-byte store each
//   tail   codeword bytes [h + 240, 255)    the last 15 - h bytes
// so every row is 15 full windows and 15 edge bytes, whatever a.  The edge bytes go out as naturally
// aligned pieces of 1, 2, 4 and 8 bytes of their own: the head's by the bits of h in ascending order
// (it ends on a 16-byte boundary), the tail's by the bits of 15 - h in descending order (it starts on
// one) -- at most 8 pieces.  No byte outside [d, d + 255) is written and nothing of the image is
// read: the rows index[r] +- 1 share windows and cache lines with this one and may be written by
// another workgroup, or another kernel, at the same time.
//
// The tile's 1,024 slots, 4 per thread of the workgroup: slot s < 960 is full window s % 15 of row
// s / 15 (consecutive lanes, consecutive windows of a row); slot 960 + r is row r's edge, so the
// edges are the last 64 slots -- one wave's last round -- and their narrow stores are 8 wave
// instructions per tile, with every lane on a row.
// An entry idx >= image_blocks (0xFFFFFFFF among them; the entries past the list's end in the
// partial last tile are read as that) is never turned into an address and stores nothing.
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace liststore {

constexpr uint32_t ROW = 255, TILE_ROWS = 64, FULL_PER_ROW = 15;
constexpr uint32_t TILE_FULL = TILE_ROWS * FULL_PER_ROW, TILE_SLOTS = TILE_FULL + TILE_ROWS; // 960, 1,024
constexpr uint32_t EDGE_PIECES = 8, TAIL_C0 = 16 * FULL_PER_ROW;                             // tail: from byte h + 240

// slot s < TILE_FULL
struct Full {
    uint32_t row, j;
};
PPFS_HD inline Full full_slot(uint32_t s)
{
    const uint32_t row = s / FULL_PER_ROW;
    return Full { row, s - row * FULL_PER_ROW };
}

// where a row goes
struct Dst {
    bool live;  // false: the entry names no block of the image; d and h are 0
    uint64_t d; // address of codeword byte 0
    uint32_t h; // head bytes
};
// base: the image's address (any alignment)
PPFS_HD inline Dst row_dst(uint64_t base, uint64_t image_blocks, uint32_t idx)
{
    if (idx >= image_blocks)
        return Dst { false, 0, 0 };
    const uint64_t d = base + (uint64_t)idx * ROW;
    return Dst { true, d, (16u - (uint32_t)(d & 15u)) & 15u };
}

// `size` codeword bytes from byte c0 to address a (a multiple of size); size 0: no store
struct Piece {
    uint64_t a;
    uint32_t c0, size;
};

// full window j of a live row
PPFS_HD inline Piece full_piece(const Dst& x, uint32_t j)
{
    const uint32_t c0 = x.h + 16u * j;
    return Piece { x.d + c0, c0, 16u };
}

// edge piece q of a live row: q = 0..3 the head's piece of 1 << q bytes, q = 4..7 the tail's piece of
// 8 >> (q - 4) bytes
PPFS_HD inline Piece edge_piece(const Dst& x, uint32_t q)
{
    const uint32_t size = q < 4u ? 1u << q : 8u >> (q - 4u);
    const uint32_t len = q < 4u ? x.h : 15u - x.h; // head or tail bytes
    // head: the pieces below this one come first; tail: the pieces above it
    const uint32_t off = q < 4u ? len & (size - 1u) : len & ~(2u * size - 1u);
    const uint32_t c0 = (q < 4u ? 0u : x.h + TAIL_C0) + off;
    return Piece { x.d + c0, c0, (len & size) ? size : 0u };
}

} // namespace liststore
} // namespace ppfs
