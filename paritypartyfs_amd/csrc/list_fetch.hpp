#pragma once
// list_fetch.hpp -- the address plan of the list decode's row fetch (rs_wg_list.hpp): which bytes
// of the image each 16-byte window of a 64-row LDS tile is made of, and how they may be read.
// Plain arithmetic for host and device alike, so the kernel's loader and tests/cpp/test_list_fetch.cpp
// (the same plan over a heap buffer, under the address sanitizer) decide identically.
//
// The tile: row r of the tile is image row index[r], 255 bytes, rows packed back to back -- the
// layout the contiguous decode's LDS-DMA leaves, cut into 1,020 windows of 16 bytes.  Window w
// starts at tile byte 16 w = 255 row + col.  With col + 16 <= 255 it lies inside one row (interior);
// otherwise (60 windows, rows 0..62) its first n0 = 255 - col bytes are the row's tail and the rest
// the head of row + 1 (boundary).  Either piece is read as "the 16 bytes whose byte lo is byte c0 of
// image row idx": through the five aligned dwords from the one that holds byte 0 (the funnel,
// funnel.hpp; always five, so the loader's loads are the same instructions in every lane) where those
// lie inside [image, image + image_blocks * 255), else -- next to the image's two ends only -- its own
// bytes [lo, hi) one by one.  An entry idx >= image_blocks is never turned into an address.
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace listfetch {

constexpr uint32_t ROW = 255, TILE_ROWS = 64, TILE_WINDOWS = TILE_ROWS * ROW / 16; // 1,020

struct Window {
    uint32_t row, col; // the window's first byte: byte col of tile row `row`
    uint32_t n0;       // its bytes [0, n0) belong to `row` (16: interior), [n0, 16) to row + 1 from byte 0
};

PPFS_HD inline Window window_of(uint32_t w)
{
    const uint32_t P = 16u * w, row = P / ROW, col = P - row * ROW;
    return Window { row, col, col + 16u <= ROW ? 16u : ROW - col };
}

enum Kind : uint32_t { SKIP = 0, FUNNEL = 1, BYTES = 2 };
constexpr uint32_t FUNNEL_SPAN = 20;

// Window bytes [lo, hi) = bytes [c0, c0 + hi - lo) of image row idx.
struct Part {
    Kind kind;      // SKIP: idx is no block of the image, the bytes are zeros
    uint64_t p0;    // address of the window's byte 0 (byte lo is at p0 + lo); FUNNEL, BYTES
    uint32_t lo, hi;
    uint64_t a;     // FUNNEL: the aligned dwords read are [a, a + span)
    uint32_t span;
};

// base: the image's address (any alignment)
PPFS_HD inline Part plan_part(uint64_t base, uint64_t image_blocks, uint32_t idx, uint32_t c0, uint32_t lo, uint32_t hi)
{
    Part p { SKIP, 0, lo, hi, 0, 0 };
    if (idx >= image_blocks || lo >= hi)
        return p;
    const uint64_t first = base + (uint64_t)idx * ROW + c0; // the part's first byte, inside the image
    p.p0 = first - lo;
    p.a = p.p0 & ~(uint64_t)3;
    p.span = FUNNEL_SPAN;
    // p0 < base only for lo > 0 at the image's first row: then a < base as well
    const bool inside = p.p0 >= base && p.a >= base && p.a + p.span <= base + image_blocks * ROW;
    p.kind = inside ? FUNNEL : BYTES;
    return p;
}

// the two parts of window w, given the tile's two entries it may touch (idx1 is ignored for an
// interior window)
PPFS_HD inline Part part_a(uint64_t base, uint64_t image_blocks, const Window& x, uint32_t idx0)
{
    return plan_part(base, image_blocks, idx0, x.col, 0, x.n0);
}
PPFS_HD inline Part part_b(uint64_t base, uint64_t image_blocks, const Window& x, uint32_t idx1)
{
    return plan_part(base, image_blocks, idx1, 0, x.n0, 16);
}

} // namespace listfetch
} // namespace ppfs
