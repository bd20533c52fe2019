// test_list_store.cpp -- the store plan of the list encode's emission
// (paritypartyfs_amd/csrc/list_store.hpp) on the host: a tile's emission is executed slot by slot, exactly
// as the kernel (rs_wg_list.hpp list_emit_tile) goes by the plan -- 960 full windows, one 16-byte store
// each, and 64 edges of up to 8 narrow pieces -- over an image that ends exactly at the end of a heap
// allocation and starts at every alignment 0..15.  Every store goes through st(), which checks its
// alignment and bounds and counts a writer per byte; the address sanitizer sees the same stores (the
// allocation's end is the image's end, its front is poisoned by hand).  No HIP: built with the host
// compiler (tests/test_list_store_cpu.py, with the address and undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/list_store.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define PPFS_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__)
#define PPFS_ASAN 1
#endif
#ifdef PPFS_ASAN
#include <sanitizer/asan_interface.h>
#endif

using namespace ppfs::liststore;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail < 20)                                                                                           \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// An image of `blocks` rows at alignment `align` (mod 16) whose last byte is the allocation's last
struct Image {
    static constexpr size_t FRONT = 32; // poisoned bytes in front of the image (two 16-byte units)
    uint8_t* alloc = nullptr;
    uint8_t* base = nullptr;
    size_t bytes = 0, front = 0;
    std::vector<uint32_t> writers; // per image byte
    Image(size_t blocks, unsigned align)
        : bytes(blocks * ROW)
        , writers(blocks * ROW, 0)
    {
        front = FRONT + align;
        alloc = (uint8_t*)std::malloc(front + bytes); // 16-byte aligned; the image ends where it ends
        base = alloc + front;
        std::memset(base, 0, bytes); // a codeword byte is never 0 (cw_byte)
#ifdef PPFS_ASAN
        __asan_poison_memory_region(alloc, front & ~(size_t)7); // whole shadow granules in front of the image
#endif
    }
    ~Image()
    {
#ifdef PPFS_ASAN
        __asan_unpoison_memory_region(alloc, front & ~(size_t)7);
#endif
        std::free(alloc);
    }
    bool aligned_as(unsigned align) const { return ((uintptr_t)base & 15u) == align; }
};

static Image* g_img = nullptr;
static size_t g_stores16 = 0, g_narrow = 0;

// byte j of the codeword of list entry i: never 0, different for neighbouring entries and bytes
static uint8_t cw_byte(size_t i, uint32_t j) { return (uint8_t)(1 + (i * 37 + j * 101 + j / 16) % 255); }

// the only way the emulation writes the image: `size` bytes of entry i's codeword from byte c0
static void st(const Piece& p, size_t i)
{
    const uint64_t lo = (uint64_t)(uintptr_t)g_img->base, hi = lo + g_img->bytes;
    CHECK(p.size == 1 || p.size == 2 || p.size == 4 || p.size == 8 || p.size == 16);
    CHECK(p.a % p.size == 0); // every store naturally aligned: the 16-byte ones 16-byte aligned
    CHECK(p.c0 + p.size <= ROW);
    const bool inside = p.a >= lo && p.a + p.size <= hi;
    CHECK(inside);
    if (!inside)
        return;
    uint8_t* dst = (uint8_t*)(uintptr_t)p.a;
    for (uint32_t k = 0; k < p.size; ++k) {
        dst[k] = cw_byte(i, p.c0 + k);
        ++g_img->writers[(size_t)(p.a - lo) + k];
    }
    (p.size == 16 ? g_stores16 : g_narrow) += 1;
}

// the emission of one tile whose 64 entries are slot[0..63], list entries i0 + 0..63
static void emit_tile(uint64_t image_blocks, const uint32_t (&slot)[TILE_ROWS], size_t i0)
{
    const uint64_t base = (uint64_t)(uintptr_t)g_img->base;
    static_assert(TILE_SLOTS == 1024 && TILE_FULL == 960, "4 slots per thread of a 256-thread workgroup");
    for (uint32_t s = 0; s < TILE_SLOTS; ++s) {
        if (s < TILE_FULL) {
            const Full f = full_slot(s);
            CHECK(f.row < TILE_ROWS && f.j < FULL_PER_ROW && f.row * FULL_PER_ROW + f.j == s);
            const Dst x = row_dst(base, image_blocks, slot[f.row]);
            CHECK(x.live == (slot[f.row] < image_blocks));
            if (!x.live) {
                CHECK(x.d == 0 && x.h == 0); // never an address
                continue;
            }
            const Piece p = full_piece(x, f.j);
            CHECK(p.size == 16 && p.a == x.d + p.c0);
            st(p, i0 + f.row);
        } else {
            const uint32_t r = s - TILE_FULL;
            const Dst x = row_dst(base, image_blocks, slot[r]);
            if (!x.live)
                continue;
            CHECK(x.d == base + (uint64_t)slot[r] * ROW && x.h == (16 - x.d % 16) % 16);
            uint32_t edge = 0;
            for (uint32_t q = 0; q < EDGE_PIECES; ++q) {
                const Piece p = edge_piece(x, q);
                const uint32_t want = q < 4 ? 1u << q : 8u >> (q - 4);
                CHECK(p.size == 0 || p.size == want);
                CHECK(p.a == x.d + p.c0);
                if (p.size)
                    st(p, i0 + r);
                edge += p.size;
            }
            CHECK(edge == 15); // head + tail, whatever the alignment
        }
    }
}

// runs the list and checks the image: with distinct in-range entries every byte of a listed row has one
// writer and the right value, every other byte none
static void run_list(Image& img, uint64_t blocks, const std::vector<uint32_t>& list)
{
    std::fill(img.writers.begin(), img.writers.end(), 0u);
    std::memset(img.base, 0, img.bytes);
    for (size_t t0 = 0; t0 < list.size(); t0 += TILE_ROWS) {
        uint32_t slot[TILE_ROWS];
        for (uint32_t r = 0; r < TILE_ROWS; ++r)
            slot[r] = t0 + r < list.size() ? list[t0 + r] : 0xFFFFFFFFu; // past the list's end: no block
        emit_tile(blocks, slot, t0);
    }
    std::vector<long> owner(blocks, -1);
    for (size_t i = 0; i < list.size(); ++i)
        if (list[i] < blocks) {
            CHECK(owner[list[i]] < 0); // make_list gives distinct blocks
            owner[list[i]] = (long)i;
        }
    for (uint64_t b = 0; b < blocks; ++b)
        for (uint32_t j = 0; j < ROW; ++j) {
            const size_t at = (size_t)b * ROW + j;
            if (owner[b] < 0) {
                CHECK(img.writers[at] == 0 && img.base[at] == 0);
            } else {
                CHECK(img.writers[at] == 1);
                CHECK(img.base[at] == cw_byte((size_t)owner[b], j));
            }
        }
}

// distinct in-range blocks -- block 0, the last block and runs of adjacent blocks among them -- with
// out-of-range entries in between, at the start, around the tile boundary and at the end
static std::vector<uint32_t> make_list(size_t n, uint64_t blocks, unsigned seed)
{
    const uint32_t oob[] = { (uint32_t)blocks, (uint32_t)blocks + 7u, 1u << 31, 0xFFFFFFFFu };
    std::vector<uint32_t> order; // seed 0: ascending (adjacent rows back to back); 1: last block first, descending
    for (uint64_t b = 0; b < blocks; ++b)
        order.push_back((uint32_t)(seed % 2 ? blocks - 1 - b : b));
    if (seed >= 2 && blocks > 2) { // block 0, the last block, then the even and the odd blocks
        order.clear();
        order.push_back(0);
        order.push_back((uint32_t)blocks - 1);
        for (uint64_t b = 2; b + 1 < blocks; b += 2)
            order.push_back((uint32_t)b);
        for (uint64_t b = 1; b + 1 < blocks; b += 2)
            order.push_back((uint32_t)b);
    }
    std::vector<uint32_t> v(n);
    size_t next = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool out = n > 1 ? (i == 3 || i == 62 || i == 63 || i == 64 || i + 1 == n) && seed != 0 : seed >= 2;
        if (out || next >= order.size())
            v[i] = oob[(i + seed) % 4];
        else
            v[i] = order[next++];
    }
    return v;
}

int main()
{
    for (uint64_t blocks : { (uint64_t)1, (uint64_t)2, (uint64_t)70 })
        for (unsigned align = 0; align < 16; ++align) {
            Image img(blocks, align);
            CHECK(img.aligned_as(align));
            g_img = &img;
            for (size_t n : { (size_t)1, (size_t)63, (size_t)64, (size_t)65 })
                for (unsigned seed = 0; seed < 4u; ++seed)
                    run_list(img, blocks, make_list(n, blocks, seed));
            // an image of 2^32 blocks or more would make 0xFFFFFFFF a block; here it never is one
            CHECK(!row_dst((uint64_t)(uintptr_t)img.base, blocks, 0xFFFFFFFFu).live);
            CHECK(!row_dst((uint64_t)(uintptr_t)img.base, blocks, (uint32_t)blocks).live);
            // every alignment of a row occurs among 16 consecutive blocks: a in 0..15 <-> h = (16 - a) % 16
            if (blocks >= 16) {
                unsigned seen = 0;
                for (uint32_t b = 0; b < 16; ++b)
                    seen |= 1u << row_dst((uint64_t)(uintptr_t)img.base, blocks, b).h;
                CHECK(seen == 0xFFFFu);
            }
            g_img = nullptr;
        }
    // an image with no block at all: every entry is out of range, nothing is stored
    {
        Image img(1, 5);
        g_img = &img;
        const size_t before = g_stores16 + g_narrow;
        uint32_t slot[TILE_ROWS];
        for (uint32_t r = 0; r < TILE_ROWS; ++r)
            slot[r] = r;
        emit_tile(0, slot, 0);
        CHECK(g_stores16 + g_narrow == before);
        for (uint32_t w : img.writers)
            CHECK(w == 0);
        g_img = nullptr;
    }
    CHECK(g_stores16 > 0 && g_narrow > 0);
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED (%zu 16-byte stores, %zu narrow stores)\n", g_stores16, g_narrow);
    return 0;
}
