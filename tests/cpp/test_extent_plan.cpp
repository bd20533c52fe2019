// test_extent_plan.cpp -- the byte-extent calls' arithmetic (paritypartyfs_amd/csrc/extent_plan.hpp) on
// the host: the clamp of an entry's length, the three invalidity rules at their boundary values, the
// staging layout, the entries of a readFile / writeFile walk against a literal restatement of the
// reference's loop, the runs of a list with a repeated block, and the CPU pack / overlay on guarded
// buffers.  No HIP: built with the host compiler (tests/test_extent_cpu.py, with the address and
// undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/extent_plan.hpp"

#include <cstdio>

using namespace ppfs::extplan;
namespace lp = ppfs::listplan;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

static ppfs_ecc_extent ext(uint64_t pos, uint32_t block, uint32_t offset, uint32_t length)
{
    return ppfs_ecc_extent { pos, block, (uint16_t)offset, (uint16_t)length };
}

static void test_layout_of_an_entry()
{
    static_assert(sizeof(ppfs_ecc_extent) == 16, "ppfs_ecc_extent is 16 bytes");
    const ppfs_ecc_extent e = ext(0x0102030405060708ull, 0x11121314u, 0x2122, 0x3132);
    uint8_t b[16];
    std::memcpy(b, &e, 16);
    const uint8_t want[16] = { 8, 7, 6, 5, 4, 3, 2, 1, 0x14, 0x13, 0x12, 0x11, 0x22, 0x21, 0x32, 0x31 };
    CHECK(std::memcmp(b, want, 16) == 0); // pos, block, offset, length; little endian, no padding
}

static void test_clamp()
{
    const size_t ds = 249;
    CHECK(eff_len(0, 249, ds) == 249);
    CHECK(eff_len(0, 250, ds) == 249);
    CHECK(eff_len(0, 0xFFFF, ds) == 249);
    CHECK(eff_len(0, 0, ds) == 0);
    CHECK(eff_len(1, 249, ds) == 248);
    CHECK(eff_len(248, 1, ds) == 1);
    CHECK(eff_len(248, 5, ds) == 1);
    CHECK(eff_len(249, 5, ds) == 0); // offset == dataSize(): zero bytes
    CHECK(eff_len(250, 5, ds) == 0);
    CHECK(eff_len(0, 7, 0) == 0); // a codec without payload bytes: nothing divides by ds
    CHECK(eff_len(100, 33, 4096) == 33);
    CHECK(eff_len(4095, 0xFFFF, 4096) == 1);
}

static void test_validity()
{
    const size_t blocks = 96, ds = 249, bytes = 1000;
    // block
    CHECK(valid(ext(0, 95, 0, 10), blocks, ds, bytes));
    CHECK(!valid(ext(0, 96, 0, 10), blocks, ds, bytes));
    CHECK(!valid(ext(0, 0xFFFFFFFFu, 0, 10), blocks, ds, bytes));
    CHECK(!valid(ext(0, 0, 0, 0), 0, ds, bytes));
    // 0xFFFFFFFF names no block, however large the image
    CHECK(!valid(ext(0, 0xFFFFFFFFu, 0, 10), (size_t)1 << 33, ds, bytes));
    CHECK(valid(ext(0, 0xFFFFFFFEu, 0, 10), (size_t)1 << 33, ds, bytes));
    CHECK(image_blocks_seen((size_t)1 << 33) == 0xFFFFFFFFu && image_blocks_seen(96) == 96);
    // offset
    CHECK(valid(ext(0, 3, 249, 10), blocks, ds, bytes)); // zero bytes at the payload's end
    CHECK(valid(ext(1000, 3, 249, 10), blocks, ds, bytes)); // ... anywhere up to the buffer's end
    CHECK(!valid(ext(0, 3, 250, 10), blocks, ds, bytes));
    CHECK(!valid(ext(0, 3, 250, 0), blocks, ds, bytes));
    // pos + len against the packed buffer, with the CLAMPED length
    CHECK(valid(ext(990, 3, 0, 10), blocks, ds, bytes));
    CHECK(!valid(ext(991, 3, 0, 10), blocks, ds, bytes));
    CHECK(valid(ext(999, 3, 248, 10), blocks, ds, bytes)); // clamped to 1 byte
    CHECK(!valid(ext(1000, 3, 248, 10), blocks, ds, bytes));
    CHECK(valid(ext(1000, 3, 0, 0), blocks, ds, bytes));
    CHECK(!valid(ext(1001, 3, 0, 0), blocks, ds, bytes));
    CHECK(!valid(ext(~0ull, 3, 0, 10), blocks, ds, bytes)); // pos + len wraps
    CHECK(!valid(ext(~0ull - 4, 3, 0, 10), blocks, ds, bytes));
    CHECK(valid(ext(0, 3, 0, 0), blocks, ds, 0));
    CHECK(!valid(ext(0, 3, 0, 1), blocks, ds, 0));
    // ds == 0: every entry is zero-length
    CHECK(valid(ext(0, 3, 0, 77), blocks, 0, 0));
    CHECK(!valid(ext(0, 3, 1, 77), blocks, 0, 0));
    CHECK(staged_index(ext(0, 95, 0, 10), blocks, ds, bytes) == 95);
    CHECK(staged_index(ext(0, 96, 0, 10), blocks, ds, bytes) == kNoBlock);
}

static void test_stage_layout()
{
    for (size_t ds : { (size_t)0, (size_t)1, (size_t)249, (size_t)4096 })
        for (size_t piece : { (size_t)1024, (size_t)65536 }) {
            const ExtStageLayout L = ext_stage_layout(piece, ds);
            CHECK(L.payload == 0 && L.index % 16 == 0 && L.index >= piece * ds && L.index >= 16);
            CHECK(L.total >= L.index + piece * 4);
        }
}

// FileIO::readFile's loop (file_io.cpp:24-42), restated: from `offset`, block by block, the bytes of
// one block at a time until bytes_to_read are read
static std::vector<ppfs_ecc_extent> reference_walk(const std::vector<uint32_t>& blocks, size_t offset, size_t bytes_to_read,
    size_t ds)
{
    std::vector<ppfs_ecc_extent> out;
    size_t offset_in_block = offset % ds, read = 0, it = 0;
    while (read < bytes_to_read && it < blocks.size()) {
        const size_t to_read = std::min(ds - offset_in_block, bytes_to_read - read);
        out.push_back(ext(read, blocks[it++], (uint32_t)offset_in_block, (uint32_t)to_read));
        read += to_read;
        offset_in_block = 0;
    }
    return out;
}

static bool same(const std::vector<ppfs_ecc_extent>& a, const std::vector<ppfs_ecc_extent>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(ppfs_ecc_extent)) == 0);
}

static void test_file_extents()
{
    std::vector<uint32_t> blocks;
    for (uint32_t k = 0; k < 41; ++k)
        blocks.push_back((k * 37u + 5u) % 96u);
    std::vector<ppfs_ecc_extent> got;
    for (size_t ds : { (size_t)249, (size_t)2, (size_t)4096 })
        for (size_t off0 : { (size_t)0, (size_t)1, ds - 1 })
            for (size_t tail : { (size_t)1, ds - 1, ds }) {
                if (tail == 0)
                    continue;
                for (size_t middle : { (size_t)0, (size_t)1, (size_t)39 }) {
                    const size_t nbytes = (ds - off0) + middle * ds + tail;
                    const size_t covered = file_extents(blocks.data(), blocks.size(), off0, nbytes, ds, got);
                    CHECK(covered == nbytes);
                    CHECK(got.size() == middle + 2);
                    CHECK(same(got, reference_walk(blocks, 7 * ds + off0, nbytes, ds)));
                    CHECK(got.front().offset == off0 && got.front().length == ds - off0 && got.front().pos == 0);
                    CHECK(got.back().offset == 0 && got.back().length == tail && got.back().pos + tail == nbytes);
                }
            }
    // the single-block file: head = tail
    CHECK(file_extents(blocks.data(), 1, 3, 5, 249, got) == 5);
    CHECK(got.size() == 1 && got[0].pos == 0 && got[0].block == blocks[0] && got[0].offset == 3 && got[0].length == 5);
    CHECK(same(got, reference_walk({ blocks[0] }, 3, 5, 249)));
    // more bytes than blocks: the walk stops with the blocks
    CHECK(file_extents(blocks.data(), 2, 10, 10000, 249, got) == 239 + 249 && got.size() == 2);
    CHECK(file_extents(blocks.data(), 2, 0, 0, 249, got) == 0 && got.empty());
    CHECK(file_extents(blocks.data(), 2, 0, 10, 0, got) == 0 && got.empty()); // no payload bytes: nothing to walk
    CHECK(file_extents(blocks.data(), 2, 249, 10, 249, got) == 0 && got.empty());
}

static void test_runs_with_a_repeated_block()
{
    const size_t blocks = 96, ds = 249, bytes = 64;
    // two inode updates in block 5, an invalid entry naming block 5 too (touches nothing), block 5 again
    const std::vector<ppfs_ecc_extent> e = { ext(0, 5, 0, 8), ext(8, 9, 4, 8), ext(16, 5, 4, 8), ext(60, 5, 0, 8),
        ext(24, 5, 250, 8), ext(24, 7, 0, 8), ext(32, 5, 8, 8), ext(40, 96, 0, 8) };
    std::vector<uint32_t> ix;
    for (const auto& x : e)
        ix.push_back(staged_index(x, blocks, ds, bytes));
    const std::vector<uint32_t> want = { 5, 9, 5, kNoBlock, kNoBlock, 7, 5, kNoBlock };
    CHECK(ix == want);
    std::vector<size_t> cuts;
    for (size_t s = 0; s < ix.size();) {
        const size_t end = lp::run_end(ix.data(), ix.size(), s, image_blocks_seen(blocks), 1000);
        CHECK(end > s);
        if (end <= s)
            break;
        cuts.push_back(end);
        s = end;
    }
    const std::vector<size_t> want_cuts = { 2, 6, 8 }; // cut where VALID block 5 repeats; invalid entries cut nothing
    CHECK(cuts == want_cuts);
}

static void test_pack_and_overlay()
{
    const size_t ds = 37, m = 6, guard = 32, bytes = 100;
    std::vector<uint8_t> P(m * ds);
    for (size_t i = 0; i < P.size(); ++i)
        P[i] = (uint8_t)(i * 7 + 1);
    const std::vector<ppfs_ecc_extent> e = { ext(0, 1, 0, 37), ext(37, 2, 36, 9), ext(40, 3, 5, 17), ext(57, 4, 37, 3),
        ext(60, 5, 3, 20), ext(95, 6, 1, 5) };
    const std::vector<uint32_t> ix = { 1, 2, 3, 4, kNoBlock, 6 };
    const std::vector<uint8_t> st = { 0, 1, 5, 0, 0, 0 };
    // exactly guard + bytes + guard bytes: the address sanitizer sees any access past them
    std::vector<uint8_t> buf(guard + bytes + guard, 0xA5), want(buf);
    pack_cpu(P.data(), ds, e.data(), ix.data(), st.data(), m, buf.data() + guard);
    std::memcpy(want.data() + guard + 0, P.data(), 37);
    want[guard + 37] = P[1 * ds + 36];            // clamped to one byte
    std::memset(want.data() + guard + 40, 0, 17); // status 5: zeros
    // entry 3: zero bytes; entry 4: invalid, skipped
    std::memcpy(want.data() + guard + 95, P.data() + 5 * ds + 1, 5); // ends at the buffer's end
    CHECK(buf == want);
    // without a status array nothing is zeroed
    std::vector<uint8_t> buf2(guard + bytes + guard, 0xA5);
    pack_cpu(P.data(), ds, e.data(), ix.data(), nullptr, m, buf2.data() + guard);
    CHECK(std::memcmp(buf2.data() + guard + 40, P.data() + 2 * ds + 5, 17) == 0);

    std::vector<uint8_t> in(bytes);
    for (size_t i = 0; i < in.size(); ++i)
        in[i] = (uint8_t)(200 - i);
    std::vector<uint8_t> Q(m * ds, 0xA5), wantQ(Q);
    overlay_cpu(in.data(), e.data(), ix.data(), m, Q.data(), ds);
    std::memcpy(wantQ.data(), in.data(), 37);
    wantQ[1 * ds + 36] = in[37];
    std::memcpy(wantQ.data() + 2 * ds + 5, in.data() + 40, 17);
    std::memcpy(wantQ.data() + 5 * ds + 1, in.data() + 95, 5);
    CHECK(Q == wantQ);
    // ds == 0: nothing moves, nothing is dereferenced
    pack_cpu(nullptr, 0, e.data(), ix.data(), st.data(), m, nullptr);
    overlay_cpu(nullptr, e.data(), ix.data(), m, nullptr, 0);
}

int main()
{
    test_layout_of_an_entry();
    test_clamp();
    test_validity();
    test_stage_layout();
    test_file_extents();
    test_runs_with_a_repeated_block();
    test_pack_and_overlay();
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
