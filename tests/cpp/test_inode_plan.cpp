// test_inode_plan.cpp -- the arithmetic of the inode reads (paritypartyfs_amd/csrc/inode_plan.hpp) on the host,
// against a literal restatement of the reference's loops: InodeManager::_getInodeLocation and _readInode's
// two-branch loop over a clamping readBlock (lib/inode_manager/src/inode_manager.cpp:11-18, 56-89,
// rs_block_device.cpp:28-48), Bitmap::_getByteLocation / getBit (lib/bitmap/src/bitmap.cpp:8-14, 87-101) and
// InodeManager::get's order of evaluation (:127-138).  Every inode of a table for ds in {1, 2, 3, 27, 31, 79, 80, 81,
// 82, 162, 249, 4091, 4095, 65535}, inode numbers near 2^32, the piece size of the device call, the status rule over
// every combination of statuses of a short inode and random ones of a long one, the shared epilogue (bitmap_step,
// inode_status) against a restatement of its former copies with the piece_status row in a heap buffer of exactly 1 + K
// bytes, slot_of and the read's extents against piece(), and the row split over a heap buffer of exactly 81 bytes.
// No HIP: built with the host compiler (tests/test_inodes_cpu.py, with the address and
// undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/inode_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ppfs::inodeplan;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail < 20)                                                                                           \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// ---- the reference, restated ----
constexpr uint64_t kInode = 81; // sizeof(Inode), packed
struct DataLocation {
    uint64_t block_index, offset;
};
struct Read { // one readBlock(location, length) as the device saw it, and where its bytes went
    DataLocation at;
    uint64_t asked, got, into;
};
static DataLocation getInodeLocation(uint64_t table, uint64_t inode, uint64_t ds)
{
    DataLocation result;
    result.block_index = table + inode * kInode / ds;
    result.offset = inode * kInode % ds;
    return result;
}
// readBlock clamps: bytes_to_read = min(ds - offset, asked), and resizes the vector to that
static uint64_t readBlock(const DataLocation& at, uint64_t asked, uint64_t ds) { return asked < ds - at.offset ? asked : ds - at.offset; }
static std::vector<Read> readInode(uint64_t table, uint64_t index, uint64_t ds)
{
    std::vector<Read> reads;
    uint64_t bytes_read = 0;
    DataLocation start = getInodeLocation(table, index, ds);
    if (ds - start.offset < kInode) {
        const uint64_t got = readBlock(start, kInode, ds);
        reads.push_back(Read { start, kInode, got, 0 });
        start.offset = 0;
        start.block_index++;
        bytes_read += got;
    }
    while (bytes_read < kInode) {
        const uint64_t bytes_left = kInode - bytes_read;
        const uint64_t got = readBlock(start, bytes_left, ds);
        reads.push_back(Read { start, bytes_left, got, bytes_read });
        bytes_read += got;
        start.block_index++;
    }
    return reads;
}
static DataLocation getByteLocation(uint64_t start_block, uint64_t bit_index, uint64_t ds)
{
    const uint64_t byte = bit_index / 8;
    const uint64_t block = byte / ds;
    const uint64_t offset = byte % ds;
    return { start_block + block, offset };
}
static bool getBit(uint8_t byte, uint64_t bit_index)
{
    const uint64_t bit = bit_index % 8;
    return ((byte >> (7 - bit)) & 1) > 0;
}

static void check_inode(uint32_t table, uint32_t bitmap, uint64_t ino, uint64_t ds)
{
    const std::vector<Read> ref = readInode(table, ino, ds);
    const uint32_t np = pieces(ino, ds), K = max_pieces(ds);
    CHECK(np == ref.size());
    CHECK(np >= 1 && np <= K);
    uint64_t covered = 0;
    for (uint32_t k = 0; k < np && k < ref.size(); ++k) {
        const Piece p = piece(table, ino, k, ds);
        CHECK(p.block == ref[k].at.block_index);
        CHECK(p.offset == ref[k].at.offset);
        CHECK(p.length == ref[k].got);
        CHECK(p.pos == ref[k].into);
        CHECK(p.pos == covered && p.length >= 1 && p.offset + (uint64_t)p.length <= ds);
        covered += p.length;
    }
    CHECK(covered == kInode);
    const DataLocation loc = getByteLocation(bitmap, ino, ds);
    const BitByte b = bitmap_byte(bitmap, ino, ds);
    CHECK(b.block == loc.block_index && b.offset == loc.offset && b.offset < ds);
    for (unsigned byte = 0; byte < 256; byte += 51) // 0x00, 0x33, 0x66, 0x99, 0xCC, 0xFF
        CHECK(((byte & b.mask) != 0) == getBit((uint8_t)byte, ino));
    CHECK(b.mask == (0x80u >> (ino % 8)));
    // slot_of and the read's extent of a slot against piece(): entry j = 5 of a piece
    struct Ext {
        uint64_t pos;
        uint32_t block;
        uint16_t offset, length;
    };
    for (uint32_t k = 0; k < K; ++k) {
        const Slot s = slot_of(table, (uint32_t)ino, k, 0, ds);
        const Piece p = piece(table, ino, k, ds);
        CHECK(s.takes_part == (k < np && p.block < NO_BLOCK));
        const Ext e = slot_extent<Ext>(s, 5);
        if (s.takes_part) {
            CHECK(s.block == p.block && s.offset == p.offset && s.length == p.length && s.pos == p.pos);
            CHECK(e.pos == 81u * 5u + p.pos && e.block == p.block && e.offset == p.offset && e.length == p.length);
        } else {
            CHECK(e.pos == 0 && e.block == NO_BLOCK && e.offset == 0 && e.length == 0);
        }
        for (uint32_t verdict : { 5u, 9u, 255u }) {
            const Slot out = slot_of(table, (uint32_t)ino, k, verdict, ds);
            const Ext none = slot_extent<Ext>(out, 5);
            CHECK(!out.takes_part && none.pos == 0 && none.block == NO_BLOCK && none.offset == 0 && none.length == 0);
        }
    }
}

// InodeManager::get over per-read statuses, stopping at the first error: what the status rule restates
static uint32_t loop_status(uint64_t ino, uint64_t total, bool check, uint32_t bst, bool bit_set, const std::vector<uint32_t>& pst)
{
    bool corrected = false;
    if (ino >= total)
        return 9; // Bitmap_IndexOutOfRange, also without the bitmap: the table has no such inode
    if (check) {
        if (bst == 5 || bst == 9)
            return bst;
        corrected |= bst == 1;
        if (bit_set)
            return 255; // InodeManager_NotFound
    }
    for (uint32_t s : pst) {
        if (s == 5 || s == 9)
            return s;
        corrected |= s == 1;
    }
    return corrected ? 1 : 0;
}
static uint32_t plan_status(uint64_t ino, uint64_t total, bool check, uint32_t bst, uint32_t byte, uint32_t mask,
    const std::vector<uint32_t>& pst)
{
    const bool bit_read = check && ino < total;
    const uint32_t v = bitmap_verdict(ino, total, check, bst, byte, mask);
    if (v)
        return v;
    return table_status(bit_read ? bst : 0u, (uint32_t)pst.size(), [&](uint32_t k) {
        CHECK(k < pst.size());
        return pst[k];
    });
}

static void check_status_rule()
{
    const uint32_t codes[4] = { 0, 1, 5, 9 };
    uint32_t rng = 12345;
    auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 16; };
    for (int check = 0; check < 2; ++check)
        for (uint64_t ino : { 3ull, 10ull, 11ull })             // total 11: the last inode, and one past
            for (uint32_t bst : codes)
                for (int bit = 0; bit < 2; ++bit)
                    for (uint32_t np = 1; np <= 3; ++np)
                        for (uint32_t combo = 0; combo < 64; ++combo) {
                            std::vector<uint32_t> pst(np);
                            for (uint32_t k = 0; k < np; ++k)
                                pst[k] = codes[(combo >> (2 * k)) & 3];
                            const uint32_t mask = 0x80u >> (ino % 8), byte = bit ? 0xFFu : (0xFFu & ~mask);
                            CHECK(plan_status(ino, 11, check, bst, byte, mask, pst) == loop_status(ino, 11, check, bst, bit, pst));
                        }
    for (int round = 0; round < 2000; ++round) { // an inode of 81 pieces (ds = 1)
        std::vector<uint32_t> pst(81);
        for (auto& s : pst)
            s = next() % 23 == 0 ? codes[next() % 4] : 0u;
        const uint32_t bst = codes[next() % 4] * (next() % 3 == 0), byte = next() & 0xFF;
        CHECK(plan_status(5, 100, true, bst, byte, 0x04, pst) == loop_status(5, 100, true, bst, (byte & 0x04) != 0, pst));
    }
    CHECK(count_slot(0) == 0 && count_slot(1) == 1 && count_slot(5) == 2 && count_slot(9) == 3 && count_slot(255) == 4
        && count_slot(2) == -1);
}

// The epilogue as each of its four copies spelt it out (the merge and write-status kernels, the two host forms) before
// bitmap_step and inode_status held it once; pst: K piece statuses, ps: 1 + K bytes
static uint32_t old_epilogue(uint32_t ino, uint32_t total, bool check, uint32_t bst, uint32_t bm, uint64_t ds, uint32_t K,
    const std::vector<uint32_t>& pst, uint8_t* ps)
{
    const bool seen = check && ino < total && (bst == ST_OK || bst == ST_CORRECTED);
    const uint32_t v = bitmap_verdict(ino, total, check, bst, seen ? bm : 0u, 0x80u >> (ino % 8u));
    const bool bit_read = check && ino < total;
    const uint32_t np = v == 0u ? pieces(ino, ds) : 0u;
    const uint32_t st = v ? v : table_status(bit_read ? bst : 0u, np, [&](uint32_t k) { return pst[k]; });
    ps[0] = bit_read ? (uint8_t)bst : (uint8_t)ST_UNUSED;
    for (uint32_t k = 0; k < K; ++k)
        ps[1u + k] = k < np ? (uint8_t)pst[k] : (uint8_t)ST_UNUSED;
    return st;
}

static void check_one_epilogue(uint32_t ino, uint64_t ds, const std::vector<uint32_t>& pst)
{
    const uint32_t codes[4] = { 0, 1, 5, 9 }, K = max_pieces(ds), np = pieces(ino, ds);
    std::vector<uint8_t> want(1 + K);
    uint8_t* row = (uint8_t*)std::malloc(1 + K); // exactly 1 + K bytes: a store past it is the sanitizer's
    for (uint32_t total : { ino, ino + 1u })        // out of range, the last inode
        for (uint32_t check = 0; check < 2; ++check) // in the states that do not read the bit, its bytes are anything
            for (uint32_t bst : codes)
                for (int bit = 0; bit < 2; ++bit) {
                    const uint32_t mask = 0x80u >> (ino % 8), byte = bit ? 0xFFu : (0xFFu & ~mask);
                    const uint32_t old = old_epilogue(ino, total, check != 0, bst, byte, ds, K, pst, want.data());
                    auto piece_st = [&](uint32_t k) {
                        CHECK(k < np);
                        return pst[k];
                    };
                    const BitmapStep b = bitmap_step(Table { 7, 3, total, check }, ino, byte, bst);
                    std::memset(row, 0xAA, 1 + K);
                    CHECK(inode_status(b, ino, ds, K, piece_st, row) == old);
                    CHECK(std::memcmp(row, want.data(), 1 + K) == 0);
                    CHECK(inode_status(b, ino, ds, K, piece_st, nullptr) == old);
                    CHECK(b.bit_read == (ino < total && check) && b.bitmap_status == want[0]);
                    CHECK(old == loop_status(ino, total, check != 0, bst, bit != 0, std::vector<uint32_t>(pst.begin(), pst.begin() + np)));
                }
    std::free(row);
}

// K in {2, 3, 4, 81}: every bitmap state with every combination of piece statuses of the inodes of one to four
// pieces, and with random ones of the inode of 81
static void check_epilogue()
{
    const uint32_t codes[4] = { 0, 1, 5, 9 };
    uint32_t rng = 777;
    auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 16; };
    for (uint64_t ds : { 249ull, 79ull, 31ull, 1ull }) {
        const uint32_t K = max_pieces(ds);
        CHECK(K == (ds == 249 ? 2u : ds == 79 ? 3u : ds == 31 ? 4u : 81u));
        uint32_t seen_np = 0; // a bit per piece count met
        for (uint32_t ino = 0; ino < 400; ++ino) {
            const uint32_t np = pieces(ino, ds);
            if (seen_np >> (np % 32u) & 1u)
                continue;
            seen_np |= 1u << (np % 32u);
            std::vector<uint32_t> pst(K, 9); // the slots behind the inode's pieces: never looked at
            if (np <= 4) {
                for (uint32_t combo = 0; combo < (1u << (2 * np)); ++combo) {
                    for (uint32_t k = 0; k < np; ++k)
                        pst[k] = codes[(combo >> (2 * k)) & 3];
                    check_one_epilogue(ino, ds, pst);
                }
            } else {
                for (int round = 0; round < 500; ++round) {
                    for (uint32_t k = 0; k < np; ++k)
                        pst[k] = next() % 23 == 0 ? codes[next() % 4] : 0u;
                    check_one_epilogue(ino, ds, pst);
                }
            }
        }
        CHECK(seen_np >> (K % 32u) & 1u); // an inode of K pieces was among them
        if (ds == 249)
            CHECK(seen_np == 0x6u); // one and two pieces
    }
}

static void check_fields()
{
    uint8_t* row = (uint8_t*)std::malloc(kInode); // exactly 81 bytes: a read past it is the sanitizer's
    for (uint32_t i = 0; i < kInode; ++i)
        row[i] = (uint8_t)(i * 7 + 1);
    auto at = [&](uint32_t i) -> uint32_t {
        CHECK(i < kInode);
        return row[i];
    };
    uint64_t t0, t1;
    std::memcpy(&t0, row, 8);
    std::memcpy(&t1, row + 8, 8);
    CHECK(le64(at, 0) == t0 && le64(at, 8) == t1);
    for (uint32_t w = 0; w < FILE_BYTES / 4; ++w) {
        uint32_t v;
        std::memcpy(&v, row + FILE_OFF + 4 * w, 4);
        CHECK(le32(at, FILE_OFF + 4 * w) == v);
    }
    CHECK(FILE_OFF + FILE_BYTES == TYPE_OFF && TYPE_OFF + 1 == INODE_BYTES && at(TYPE_OFF) == row[80]);
    std::free(row);
}

int main()
{
    const uint64_t sizes[] = { 1, 2, 3, 27, 31, 79, 80, 81, 82, 162, 249, 4091, 4095, 65535 };
    for (uint64_t ds : sizes) {
        const uint32_t K = max_pieces(ds);
        CHECK(K == 2 + 79 / ds);
        CHECK((ds >= 80) == (K == 2));
        const uint64_t total = ds + 300; // every offset 81 i % ds occurs
        uint32_t most = 0;
        for (uint64_t ino = 0; ino < total; ++ino) {
            check_inode(7, 3, ino, ds);
            most = pieces(ino, ds) > most ? pieces(ino, ds) : most;
        }
        CHECK(most <= K);
        if (ds % 3 != 0)
            CHECK(most == K); // gcd(81, ds) = 1: some inode starts at the last byte of a block
        // near 2^32, with table and bitmap blocks that carry the sum past 32 bits
        for (uint64_t ino = 0xFFFFFF00ull; ino <= 0xFFFFFFFFull; ++ino) {
            check_inode(0, 0, ino, ds);
            check_inode(0xFFFFFFF0u, 0xFFFFFFFFu, ino, ds);
        }
        const Piece far = piece(0xFFFFFFF0u, 0xFFFFFFFFull, 0, ds);
        CHECK(far.block == 0xFFFFFFF0ull + 81ull * 0xFFFFFFFFull / ds && far.block >= NO_BLOCK);
        // a piece of the device call: its extents fit one piece of the extent stream
        CHECK(piece_inodes(ds) >= 1 && piece_inodes(ds) * K <= 2 * PIECE_INODES && piece_inodes(ds) <= PIECE_INODES);
    }
    CHECK(max_pieces(31) == 4 && max_pieces(1) == 81 && max_pieces(80) == 2 && max_pieces(79) == 3);
    CHECK(pieces(3, 249) == 2 && pieces(0, 249) == 1); // 243 + 80 = 323: every fourth inode straddles
    check_status_rule();
    check_epilogue();
    check_fields();
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
