// test_list_plan.cpp -- the block-list calls' arithmetic (paritypartyfs_amd/csrc/list_plan.hpp) on the
// host: the range check of an entry, the pieces of a device call, the cut of a host list into runs
// without a repeated index, the CPU gather and the choice of rows a run copies back.  No HIP: built
// with the host compiler (tests/test_list_cpu.py, with the address and undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/list_plan.hpp"

#include <cstdio>
#include <numeric>

using namespace ppfs::listplan;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// the runs of a list as [start, end) pairs
static std::vector<std::pair<size_t, size_t>> runs(const std::vector<uint32_t>& ix, size_t image_blocks, size_t max_run)
{
    std::vector<std::pair<size_t, size_t>> out;
    for (size_t s = 0; s < ix.size();) {
        const size_t e = run_end(ix.data(), ix.size(), s, image_blocks, max_run);
        CHECK(e > s && e <= ix.size()); // a run always advances
        if (e <= s)
            break;
        out.push_back({ s, e });
        s = e;
    }
    return out;
}

static void test_range()
{
    const size_t blocks = 96;
    CHECK(in_range(0, blocks));
    CHECK(in_range((uint32_t)blocks - 1, blocks));
    CHECK(!in_range((uint32_t)blocks, blocks));
    CHECK(!in_range(0xFFFFFFFFu, blocks));
    CHECK(!in_range(0, 0));
    // an image of 2^32 blocks or more: every 32-bit index is a block of it
    CHECK(in_range(0xFFFFFFFFu, (size_t)1 << 32));
    CHECK(!in_range(0xFFFFFFFFu, ((size_t)1 << 32) - 1));
}

static void test_pieces()
{
    CHECK(piece_blocks(65536, 255) == 65536);
    CHECK(piece_blocks(4096, 4096) == 4096);
    CHECK(piece_blocks(1500, 255) == 1024); // an override that is no multiple of 1 Ki
    CHECK(piece_blocks(1, 1) == 1024);
    for (size_t raw : { (size_t)1, (size_t)255, (size_t)4096 })
        for (size_t chunk : { (size_t)1024, (size_t)65536, (size_t)1 << 22 }) {
            const size_t p = piece_blocks(chunk, raw);
            CHECK(p % 1024 == 0 && p >= 1024 && p <= std::max<size_t>(chunk, 1024));
            CHECK((uint64_t)p * raw < (1ull << 32)); // the kernels' 32-bit byte positions
            const StageLayout L = stage_layout(p, raw);
            CHECK(L.rows == 0 && L.status % 16 == 0 && L.status >= ((p * raw + 15) & ~(size_t)15));
            CHECK(L.total >= L.status + p);
        }
}

static void test_runs()
{
    const size_t blocks = 100;
    { // no duplicate: one run, or runs of max_run
        std::vector<uint32_t> ix(41);
        std::iota(ix.begin(), ix.end(), 7u);
        auto r = runs(ix, blocks, 1000);
        CHECK(r.size() == 1 && r[0].first == 0 && r[0].second == 41);
        r = runs(ix, blocks, 16);
        CHECK(r.size() == 3 && r[0].second == 16 && r[1].second == 32 && r[2].second == 41);
    }
    { // adjacent duplicates: each repeat starts a run
        const std::vector<uint32_t> ix { 5, 5, 5, 6, 7, 7 };
        const auto r = runs(ix, blocks, 1000);
        CHECK(r.size() == 4);
        CHECK(r[0] == std::make_pair((size_t)0, (size_t)1) && r[1] == std::make_pair((size_t)1, (size_t)2));
        CHECK(r[2] == std::make_pair((size_t)2, (size_t)5) && r[3] == std::make_pair((size_t)5, (size_t)6));
    }
    { // a duplicate farther apart than one run: the length limit already separated the two
        std::vector<uint32_t> ix(40);
        std::iota(ix.begin(), ix.end(), 0u);
        ix[35] = 2;
        auto r = runs(ix, blocks, 16);
        CHECK(r.size() == 3 && r[0].second == 16 && r[1].second == 32 && r[2].second == 40);
        r = runs(ix, blocks, 1000); // without the limit the repeat cuts
        CHECK(r.size() == 2 && r[0].second == 35 && r[1].second == 40);
    }
    { // out-of-range entries never cut, however often they repeat
        const std::vector<uint32_t> ix { 1, 100, 100, 0xFFFFFFFFu, 0xFFFFFFFFu, 2, 1 };
        const auto r = runs(ix, blocks, 1000);
        CHECK(r.size() == 2 && r[0].second == 6 && r[1].second == 7);
    }
    { // no run holds an in-range index twice, and the runs tile the list
        std::vector<uint32_t> ix;
        uint32_t x = 12345;
        for (int i = 0; i < 500; ++i) {
            x = x * 1664525u + 1013904223u;
            ix.push_back((x >> 16) % 120); // some out of range
        }
        size_t next = 0;
        for (auto [s, e] : runs(ix, blocks, 64)) {
            CHECK(s == next && e - s <= 64);
            next = e;
            std::unordered_set<uint32_t> seen;
            for (size_t i = s; i < e; ++i)
                if (in_range(ix[i], blocks))
                    CHECK(seen.insert(ix[i]).second);
            if (e < ix.size() && e - s < 64)
                CHECK(seen.count(ix[e]) == 1); // maximal: it ended at a repeat
        }
        CHECK(next == ix.size());
    }
    CHECK(run_end(nullptr, 0, 0, blocks, 16) == 0);
}

static void test_gather_and_copy_back()
{
    const size_t blocks = 8, raw = 5;
    std::vector<uint8_t> image(blocks * raw);
    for (size_t i = 0; i < image.size(); ++i)
        image[i] = (uint8_t)(i + 1);
    const std::vector<uint32_t> ix { 7, 0, 8, 3, 0xFFFFFFFFu };
    std::vector<uint8_t> rows(ix.size() * raw, 0xEE);
    gather_rows_cpu(image.data(), blocks, ix.data(), ix.size(), raw, rows.data());
    for (size_t i = 0; i < ix.size(); ++i)
        for (size_t b = 0; b < raw; ++b)
            CHECK(rows[i * raw + b] == (in_range(ix[i], blocks) ? image[ix[i] * raw + b] : 0));

    const std::vector<uint8_t> st { 1, 0, 1, 5, 1 };
    using V = std::vector<uint32_t>;
    CHECK(copy_back_list(OP_DECODE, true, ix.data(), ix.size(), blocks, st.data()) == V({ 0 }));
    CHECK(copy_back_list(OP_DECODE, false, ix.data(), ix.size(), blocks, st.data()).empty());
    CHECK(copy_back_list(OP_WRITE, false, ix.data(), ix.size(), blocks, st.data()) == V({ 0, 1 }));
    CHECK(copy_back_list(OP_ENCODE, false, ix.data(), ix.size(), blocks, nullptr) == V({ 0, 1, 3 }));
    CHECK(!copies_back(OP_ENCODE, false, (uint32_t)blocks, blocks, 0));
    CHECK(copies_back(OP_ENCODE, false, (uint32_t)blocks - 1, blocks, 0));

    std::vector<uint8_t> status(st), data(ix.size() * 3, 0x55);
    mark_out_of_range(ix.data(), ix.size(), blocks, status.data(), data.data(), 3);
    CHECK(status == std::vector<uint8_t>({ 1, 0, 9, 5, 9 }));
    for (size_t i = 0; i < ix.size(); ++i)
        for (size_t b = 0; b < 3; ++b)
            CHECK(data[i * 3 + b] == (in_range(ix[i], blocks) ? 0x55 : 0));
    mark_out_of_range(ix.data(), ix.size(), blocks, nullptr, nullptr, 3); // absent outputs
}

int main()
{
    test_range();
    test_pieces();
    test_runs();
    test_gather_and_copy_back();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
