// test_files_write_plan.cpp -- the write side of csrc/files_plan.hpp against brute force: the strict range rule of a
// batch write (offset + nbytes <= file_size, nothing clamped) and the detector of two ranges of one inode record
// that share a file block.  A plain host program: built with g++ -fsanitize=address,undefined by
// tests/test_file_write_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../paritypartyfs_amd/csrc/file_plan.hpp"
#include "../../paritypartyfs_amd/csrc/files_plan.hpp"

using namespace ppfs::fileplan;
namespace fp = ppfs::filesplan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (++g_fail <= 20) {                                                                                      \
                std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond);                                             \
                std::printf(__VA_ARGS__);                                                                              \
                std::printf("\n");                                                                                     \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static uint32_t g_seed = 4711;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }
static uint64_t rnd_below(uint64_t n) { return n ? (((uint64_t)rnd() << 16) ^ rnd()) % n : 0; }

struct Batch {
    std::vector<uint32_t> recs;   // 16 dwords per file
    std::vector<uint64_t> ranges; // (offset, nbytes) per file
    uint64_t n() const { return ranges.size() / 2; }
    void add(const uint32_t* rec, uint64_t offset, uint64_t nbytes)
    {
        recs.insert(recs.end(), rec, rec + 16);
        ranges.push_back(offset);
        ranges.push_back(nbytes);
    }
};

// brute force: the first file either rule refuses, and which rule
static int brute_range(const Batch& b, uint64_t ds, bool whole, uint64_t* bad)
{
    for (uint64_t f = 0; f < b.n(); ++f) {
        const uint64_t size = b.recs[16 * f + 15], off = whole ? 0 : b.ranges[2 * f], nb = whole ? size : b.ranges[2 * f + 1];
        if (nb == 0)
            continue;
        *bad = f;
        if (off + nb < off || off + nb > size)
            return fp::BAD_PAST_END;
        const uint64_t first = off / ds, count = (off % ds + nb + ds - 1) / ds;
        if (first + count > capacity(ds))
            return fp::BAD_CAPACITY;
    }
    return fp::RANGE_OK;
}

// brute force over all pairs: the smallest f with an earlier g of the same record and an intersecting span
static uint64_t brute_repeat(const Batch& b, uint64_t ds)
{
    for (uint64_t f = 0; f < b.n(); ++f) {
        const uint64_t nf = b.ranges[2 * f + 1];
        if (nf == 0)
            continue;
        const uint64_t f0 = b.ranges[2 * f] / ds, f1 = (b.ranges[2 * f] + nf - 1) / ds;
        for (uint64_t g = 0; g < f; ++g) {
            const uint64_t ng = b.ranges[2 * g + 1];
            if (ng == 0 || std::memcmp(&b.recs[16 * f], &b.recs[16 * g], 64) != 0)
                continue;
            const uint64_t g0 = b.ranges[2 * g] / ds, g1 = (b.ranges[2 * g] + ng - 1) / ds;
            if (f0 <= g1 && g0 <= f1)
                return f;
        }
    }
    return b.n();
}

static void check(const Batch& b, uint64_t ds, const char* what)
{
    fp::Plan plan;
    uint64_t bad = 99, want_bad = 99;
    const int r = fp::build_write(b.recs.data(), b.ranges.data(), b.n(), ds, plan, &bad);
    const int want = brute_range(b, ds, false, &want_bad);
    CHECK(r == want && (want == fp::RANGE_OK || bad == want_bad), "%s ds %llu: build_write %d file %llu, brute force %d file %llu", what,
        (unsigned long long)ds, r, (unsigned long long)bad, want, (unsigned long long)want_bad);
    if (r != fp::RANGE_OK || want != fp::RANGE_OK)
        return;
    // an accepted batch is never clamped: the slots are ppfs_ecc_files_plan's and hold the asked bytes
    fp::Plan read_plan;
    CHECK(fp::build(b.recs.data(), b.ranges.data(), b.n(), ds, read_plan, &bad) == fp::RANGE_OK, "%s: the read plan refuses", what);
    uint64_t at = 0;
    for (uint64_t f = 0; f < b.n(); ++f) {
        CHECK(plan.slots[f].bytes == b.ranges[2 * f + 1] && plan.slots[f].out_pos == at, "%s file %llu: bytes / out_pos", what,
            (unsigned long long)f);
        CHECK(std::memcmp(&plan.slots[f], &read_plan.slots[f], sizeof(fp::Slot)) == 0, "%s file %llu: slot differs from the read's", what,
            (unsigned long long)f);
        at += b.ranges[2 * f + 1];
    }
    const uint64_t got = fp::first_repeat(plan), brute = brute_repeat(b, ds);
    CHECK(got == brute, "%s ds %llu n %llu: first_repeat %llu, brute force %llu", what, (unsigned long long)ds, (unsigned long long)b.n(),
        (unsigned long long)got, (unsigned long long)brute);
}

int main()
{
    const uint64_t sizes[] = { 58, 2, 16, 508 };
    for (uint64_t ds : sizes) {
        // a few inode records; file sizes of some blocks
        uint32_t rec[4][16];
        for (auto& r : rec) {
            for (int d = 0; d < 15; ++d)
                r[d] = rnd();
            r[15] = (uint32_t)(ds * (3 + rnd_below(9)) + rnd_below(ds));
        }
        std::memcpy(rec[3], rec[2], 64); // two byte-identical records
        rec[1][15] = rec[0][15];         // and two that differ only in their pointers
        const uint32_t* r0 = rec[0];
        const uint64_t size = r0[15];

        { // identical records: touching, intersecting, disjoint spans
            Batch b;
            b.add(r0, 0, ds);
            b.add(r0, ds, ds); // touches block 0's end: distinct blocks
            check(b, ds, "touching");
            b.add(r0, 2 * ds - 1, 2); // the last byte of block 1 and the first of block 2
            check(b, ds, "intersecting");
        }
        {
            Batch b;
            b.add(r0, 3, 1);
            b.add(r0, ds - 1, 1); // two bytes of one block
            check(b, ds, "one block twice");
        }
        {
            Batch b;
            b.add(r0, 0, 1);
            b.add(rec[1], 0, ds); // different records, equal spans
            b.add(r0, 2 * ds, 1);
            check(b, ds, "different records");
        }
        { // the long early span hides a later pair from a sweep that looks only at the longest span so far
            Batch b;
            b.add(r0, 0, size < 2 * ds ? size : 2 * ds);
            b.add(rec[2], ds + 1, 1);
            b.add(rec[3], ds + 2, 1);
            b.add(r0, 0, size);
            check(b, ds, "later pair first");
        }
        { // empty ranges take no part, whatever their offset
            Batch b;
            b.add(r0, 5, 0);
            b.add(r0, size + 100, 0);
            b.add(r0, 0, size);
            b.add(r0, 1, 0);
            check(b, ds, "empty ranges");
        }
        { // the strict rule: one byte past the end, an offset at the end, an overflowing sum
            Batch b;
            b.add(r0, 0, size);
            b.add(rec[1], 1, size);
            check(b, ds, "one byte past the end");
            Batch c;
            c.add(r0, 0, 1);
            c.add(r0, size, 1);
            check(c, ds, "offset at the end");
            Batch d;
            d.add(r0, 3, ~0ull - 1);
            check(d, ds, "overflow");
        }
        // seeded batches of up to 40 ranges over the four records
        for (int trial = 0; trial < 3000; ++trial) {
            Batch b;
            const uint64_t n = 1 + rnd_below(40);
            const bool sparse = rnd() % 2;
            for (uint64_t f = 0; f < n; ++f) {
                const uint32_t* r = rec[rnd_below(4)];
                const uint64_t sz = r[15];
                if (rnd() % 8 == 0) {
                    b.add(r, rnd_below(2 * sz), 0);
                    continue;
                }
                const uint64_t off = rnd_below(sz), room = sz - off;
                uint64_t nb = 1 + rnd_below(sparse ? (room < ds ? room : ds) : room);
                if (rnd() % 200 == 0)
                    nb = room + 1 + rnd_below(3); // past the end
                b.add(r, off, nb);
            }
            check(b, ds, "seeded");
        }
    }
    { // ranges == NULL: every file whole, always inside the file
        uint32_t rec[32] = {};
        rec[15] = 1000;
        rec[31] = 0;
        fp::Plan plan;
        uint64_t bad = 99;
        CHECK(fp::build_write(rec, nullptr, 2, 58, plan, &bad) == fp::RANGE_OK && plan.total.bytes == 1000, "whole files");
        CHECK(fp::first_repeat(plan) == 2, "whole files: no repeat");
    }
    if (g_fail == 0)
        std::printf("ALL PASSED\n");
    else
        std::printf("%d checks failed\n", g_fail);
    return g_fail ? 1 : 0;
}
