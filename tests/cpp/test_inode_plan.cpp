// test_inode_plan.cpp -- the arithmetic of the inode reads (paritypartyfs_amd/csrc/inode_plan.hpp) on the host,
// against a literal restatement of the reference's loops: InodeManager::_getInodeLocation and _readInode's
// two-branch loop over a clamping readBlock (lib/inode_manager/src/inode_manager.cpp:11-18, 56-89,
// rs_block_device.cpp:28-48), Bitmap::_getByteLocation / getBit (lib/bitmap/src/bitmap.cpp:8-14, 87-101) and
// InodeManager::get's order of evaluation (:127-138).  Every inode of a table for ds in {1, 2, 3, 27, 31, 79, 80, 81,
// 82, 162, 249, 4091, 4095, 65535}, inode numbers near 2^32, the piece size of the device call, the status rule over
// every combination of statuses of a short inode and random ones of a long one, and the row split over a heap buffer
// of exactly 81 bytes.  No HIP: built with the host compiler (tests/test_inodes_cpu.py, with the address and
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
    check_fields();
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
