// test_list_fetch.cpp -- the address plan of the list decode's row fetch
// (paritypartyfs_amd/csrc/list_fetch.hpp) on the host: a tile fetch is emulated window by window, exactly
// as the kernel's loader (rs_wg_list.hpp) goes by the plan -- a FUNNEL part reads its 20 aligned bytes and
// shifts, a BYTES part reads its own bytes, a SKIP part reads nothing -- over an image that ends exactly
// at the end of a heap allocation and starts at every alignment 0..15.  Every read goes through rd(),
// which checks it against the image's bounds; the address sanitizer sees the same reads (the
// allocation's end is the image's end, its front is poisoned by hand).  No HIP: built with the host
// compiler (tests/test_list_direct_cpu.py, with the address and undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/list_fetch.hpp"

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

using namespace ppfs::listfetch;

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
    Image(size_t blocks, unsigned align)
        : bytes(blocks * ROW)
    {
        front = FRONT + align;
        alloc = (uint8_t*)std::malloc(front + bytes); // 16-byte aligned; the image ends where it ends
        base = alloc + front;
        for (size_t i = 0; i < bytes; ++i)
            base[i] = (uint8_t)(1 + (i * 131 + i / ROW * 7) % 255); // never 0: a zero byte is a missing read
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

static const Image* g_img = nullptr;
static size_t g_reads = 0;

// the only way the emulation reads the image
static void rd(void* dst, uint64_t addr, size_t n)
{
    const uint64_t lo = (uint64_t)(uintptr_t)g_img->base, hi = lo + g_img->bytes;
    const bool inside = addr >= lo && addr + n <= hi;
    CHECK(inside);
    if (!inside) {
        std::memset(dst, 0, n);
        return;
    }
    std::memcpy(dst, (const void*)(uintptr_t)addr, n);
    g_reads += n;
}

// window bytes [lo, hi) of a part, as the device code reads them
static void read_part(const Part& p, uint64_t base, uint64_t image_bytes, uint8_t (&out)[16])
{
    if (p.kind == SKIP)
        return;
    if (p.kind == FUNNEL) {
        CHECK(p.a % 4 == 0 && p.span == FUNNEL_SPAN && p.a <= p.p0 && p.p0 - p.a < 4);
        CHECK(p.a >= base && p.a + p.span <= base + image_bytes);
        uint32_t w[5];
        rd(w, p.a, sizeof(w)); // five aligned dwords
        uint8_t b[20];
        std::memcpy(b, w, 20);
        const uint32_t sh = (uint32_t)(p.p0 & 3u);
        for (uint32_t j = p.lo; j < p.hi; ++j)
            out[j] = b[sh + j];
        return;
    }
    // BYTES: only where the funnel's dwords would leave the image, i.e. next to its two ends
    CHECK(p.p0 < base + 3 || p.p0 + FUNNEL_SPAN > base + image_bytes);
    for (uint32_t j = p.lo; j < p.hi; ++j)
        rd(&out[j], p.p0 + j, 1);
}

static void fetch_tile(const Image& img, uint64_t image_blocks, const uint32_t (&slot)[TILE_ROWS], std::vector<uint8_t>& tile)
{
    const uint64_t base = (uint64_t)(uintptr_t)img.base;
    tile.assign(TILE_ROWS * ROW, 0xEE);
    uint32_t boundary = 0;
    for (uint32_t w = 0; w < TILE_WINDOWS; ++w) {
        const Window x = window_of(w);
        CHECK(x.row < TILE_ROWS && x.col < ROW && x.n0 >= 1 && x.n0 <= 16 && 255u * x.row + x.col == 16u * w);
        CHECK((x.n0 == 16) == (x.col + 16 <= ROW));
        uint8_t out[16] = { 0 };
        read_part(part_a(base, image_blocks, x, slot[x.row]), base, img.bytes, out);
        if (x.n0 < 16) {
            ++boundary;
            CHECK(x.row + 1 < TILE_ROWS);
            read_part(part_b(base, image_blocks, x, slot[x.row + 1]), base, img.bytes, out);
        } else {
            CHECK(part_b(base, image_blocks, x, 0).kind == SKIP); // an interior window has no second part
        }
        std::memcpy(&tile[16u * w], out, 16);
    }
    CHECK(boundary == 60); // the tile's 63 row boundaries but those at rows 16, 32, 48, where a window starts
}

static void run_list(const Image& img, uint64_t blocks, const std::vector<uint32_t>& list)
{
    std::vector<uint8_t> tile;
    for (size_t t0 = 0; t0 < list.size(); t0 += TILE_ROWS) {
        uint32_t slot[TILE_ROWS];
        for (uint32_t r = 0; r < TILE_ROWS; ++r)
            slot[r] = t0 + r < list.size() ? list[t0 + r] : 0xFFFFFFFFu; // past the list's end: no block
        fetch_tile(img, blocks, slot, tile);
        for (uint32_t r = 0; r < TILE_ROWS; ++r) {
            const uint8_t* got = &tile[(size_t)r * ROW];
            bool ok = true;
            if (slot[r] < blocks)
                ok = std::memcmp(got, img.base + (size_t)slot[r] * ROW, ROW) == 0;
            else
                for (uint32_t j = 0; j < ROW; ++j)
                    ok = ok && got[j] == 0;
            CHECK(ok);
        }
    }
}

// lists of every length asked for that hold block 0, the last block, repeats and out-of-range entries
static std::vector<uint32_t> make_list(size_t n, uint64_t blocks, unsigned seed)
{
    const uint32_t special[] = { 0u, (uint32_t)(blocks - 1), 0u, (uint32_t)blocks, (uint32_t)blocks + 5u, 0xFFFFFFFFu,
        (uint32_t)(blocks - 1), (uint32_t)(blocks / 2) };
    std::vector<uint32_t> v(n);
    uint32_t s = 12345u + seed;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        // the special entries first (a list of 1 holds one of them, chosen by the seed), and again at the
        // end of the first tile and the start of the second; seeded blocks elsewhere
        if (n == 1)
            v[i] = special[seed % 8];
        else if (i < 8)
            v[i] = special[i];
        else if (i >= 60 && i < 68)
            v[i] = special[(i + seed) % 8];
        else
            v[i] = (uint32_t)((s >> 8) % blocks);
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
                for (unsigned seed = 0; seed < (n == 1 ? 8u : 2u); ++seed)
                    run_list(img, blocks, make_list(n, blocks, seed));
            // an image of 2^32 blocks or more would make 0xFFFFFFFF a block; here it never is one
            CHECK(plan_part((uint64_t)(uintptr_t)img.base, blocks, 0xFFFFFFFFu, 0, 0, 16).kind == SKIP);
            CHECK(plan_part((uint64_t)(uintptr_t)img.base, blocks, (uint32_t)blocks, 0, 0, 16).kind == SKIP);
            g_img = nullptr;
        }
    // an image with no block at all: every entry is out of range, nothing is read
    {
        Image img(1, 5);
        g_img = &img;
        const size_t before = g_reads;
        uint32_t slot[TILE_ROWS];
        for (uint32_t r = 0; r < TILE_ROWS; ++r)
            slot[r] = r;
        std::vector<uint8_t> tile;
        fetch_tile(img, 0, slot, tile);
        CHECK(g_reads == before);
        for (uint8_t b : tile)
            CHECK(b == 0);
        g_img = nullptr;
    }
    CHECK(g_reads > 0);
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED (%zu bytes read)\n", g_reads);
    return 0;
}
