// test_inode_wplan.cpp -- the grouping step of the inode writes (paritypartyfs_amd/csrc/inode_wplan.hpp) on the host:
// the insert and lookup code the kernels run, executed serially over the slots of a piece in shuffled orders, against
// brute force.  For ds in {1, 31, 79, 80, 81, 249, 4091} and batches of a full piece (distinct numbers with some that
// do not take part, consecutive numbers, one number repeated throughout, a table that runs past block 2^32 - 2):
//   the owner of every block is the lowest slot that touches it, the winner of every number its highest entry;
//   every probe ends within the capacity, and a key that was never elected is not found;
//   the extents are one per distinct block, the overlay writes every touched byte exactly once, with the winner's
//   bytes, and the first toucher rule changes a 1 for every slot but the owner;
//   the composed 81-byte row is the packed Inode;
//   the host form's plan has the same owners and winners, and its hulls cover exactly the touched bytes.
// No HIP: built with the host compiler (tests/test_inode_write_cpu.py, with the address and undefined-behaviour
// sanitizers).
#include "../../paritypartyfs_amd/csrc/inode_wplan.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

using namespace ppfs::inodewplan;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail < 20)                                                                                           \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// the packed Inode (inode.hpp:18-41)
struct __attribute__((packed)) Inode {
    uint64_t time_creation, time_modified;
    uint32_t direct[12], indirect, doubly_indirect, trebly_indirect, file_size;
    uint8_t type;
};
static_assert(sizeof(Inode) == 81, "packed Inode");

struct Brute {
    std::map<uint32_t, uint32_t> owner;               // block -> lowest slot
    std::map<uint32_t, uint32_t> winner;              // number -> highest entry
    std::map<uint32_t, std::vector<int64_t>> writer;  // block -> per payload byte: the entry whose byte lands, -1 none
};

static Brute brute(const std::vector<uint32_t>& ino, const std::vector<uint32_t>& verdict, uint32_t table_block, uint64_t ds)
{
    Brute b;
    const uint32_t K = max_pieces(ds);
    for (size_t j = 0; j < ino.size(); ++j) { // the per-inode loop in batch order: a later write overwrites
        if (verdict[j])
            continue;
        const uint64_t byte0 = 81ull * ino[j];
        bool any = false;
        for (uint32_t i = 0; i < 81; ++i) {
            const uint64_t block = (uint64_t)table_block + (byte0 + i) / ds;
            if (block >= NO_BLOCK)
                continue;
            auto& w = b.writer[(uint32_t)block];
            if (w.empty())
                w.assign(ds, -1);
            w[(byte0 + i) % ds] = (int64_t)j;
            // the slot of this byte: the piece index is the block's distance from the inode's first block
            const uint32_t k = (uint32_t)((byte0 + i) / ds - byte0 / ds);
            CHECK(k < K);
            const uint32_t slot = (uint32_t)(j * K + k);
            auto it = b.owner.find((uint32_t)block);
            if (it == b.owner.end() || slot < it->second)
                b.owner[(uint32_t)block] = slot;
            any = any || k == 0;
        }
        if (any)
            b.winner[ino[j]] = (uint32_t)j;
    }
    return b;
}

static uint32_t g_max_steps = 0;

static void run_case(const char* what, uint64_t ds, uint32_t table_block, const std::vector<uint32_t>& ino,
    const std::vector<uint32_t>& verdict, uint32_t seed)
{
    const uint32_t K = max_pieces(ds), m = (uint32_t)ino.size(), slots = m * K;
    CHECK(m <= piece_inodes(ds) && slots <= 2 * PIECE_INODES);
    const uint32_t cap = capacity(slots);
    CHECK(cap >= 2 * slots && (cap & (cap - 1)) == 0 && cap >= 2 && (cap < 4 || cap / 2 < 2 * slots));
    std::vector<uint32_t> mem(table_bytes(cap) / 4, EMPTY); // exactly the tables: the sanitizer sees a step outside
    const Tables T = tables_at(mem.data(), cap);
    std::vector<uint32_t> order(slots);
    for (uint32_t s = 0; s < slots; ++s)
        order[s] = s;
    std::mt19937 rng(seed);
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t s : order) {
        const uint32_t j = s / K, k = s % K;
        elect<SerialOps>(T, slot_of(table_block, ino[j], k, verdict[j], ds), ino[j], j, k, s);
    }
    const Brute b = brute(ino, verdict, table_block, ds);
    // owners and winners, and the probes it takes to reach every key again
    size_t bkeys = 0, ikeys = 0;
    for (uint32_t i = 0; i < cap; ++i) {
        bkeys += T.bkey[i] != EMPTY;
        ikeys += T.ikey[i] != EMPTY;
    }
    CHECK(bkeys == b.owner.size() && ikeys == b.winner.size());
    for (auto& [block, slot] : b.owner) {
        CHECK(owner_of<SerialOps>(T, block) == slot);
        uint32_t steps = 0;
        CHECK(claim<SerialOps>(T.bkey, cap, block, &steps) != EMPTY && steps >= 1 && steps <= cap);
        g_max_steps = std::max(g_max_steps, steps);
    }
    for (auto& [number, entry] : b.winner) {
        CHECK(winner_of<SerialOps>(T, number) == entry);
        uint32_t steps = 0;
        CHECK(claim<SerialOps>(T.ikey, cap, number, &steps) != EMPTY && steps <= cap);
        g_max_steps = std::max(g_max_steps, steps);
    }
    for (uint32_t probe = 0; probe < 64; ++probe) { // keys that were never elected
        const uint32_t key = rng();
        if (key != EMPTY && !b.owner.count(key))
            CHECK(owner_of<SerialOps>(T, key) == EMPTY);
        if (key != EMPTY && !b.winner.count(key))
            CHECK(winner_of<SerialOps>(T, key) == EMPTY);
    }
    // extents: one per distinct block, at its owner slot
    size_t valid = 0;
    for (uint32_t s = 0; s < slots; ++s) {
        const Slot sl = slot_of(table_block, ino[s / K], s % K, verdict[s / K], ds);
        const bool emits = sl.takes_part && owner_of<SerialOps>(T, sl.block) == s;
        valid += emits;
        if (emits)
            CHECK(b.owner.at(sl.block) == s);
    }
    CHECK(valid == b.owner.size());
    // overlay: every touched byte has one writer, the entry the loop leaves there
    std::map<uint32_t, std::vector<int64_t>> got;
    size_t twice = 0;
    for (uint32_t s : order) {
        const uint32_t j = s / K;
        const Slot sl = slot_of(table_block, ino[j], s % K, verdict[j], ds);
        if (!sl.takes_part || winner_of<SerialOps>(T, ino[j]) != j)
            continue;
        auto& w = got[sl.block];
        if (w.empty())
            w.assign(ds, -1);
        CHECK(sl.offset + (uint64_t)sl.length <= ds && sl.pos + sl.length <= 81);
        for (uint32_t i = 0; i < sl.length; ++i) {
            twice += w[sl.offset + i] != -1;
            w[sl.offset + i] = j;
            CHECK((81ull * ino[j] + sl.pos + i) % ds == sl.offset + i);
        }
    }
    CHECK(twice == 0);
    CHECK(got == b.writer);
    // the first toucher rule
    CHECK(seen_status(1, 5, 5) == 1 && seen_status(1, 6, 5) == 0 && seen_status(5, 6, 5) == 5 && seen_status(9, 6, 5) == 9
        && seen_status(0, 6, 5) == 0);
    // the host form's plan
    const HostPlan p = plan_host(ino.data(), verdict.data(), m, table_block, ds);
    CHECK(p.groups.size() == b.owner.size() && p.group.size() == b.owner.size() && p.winner.size() == b.winner.size());
    uint32_t last_owner = 0;
    for (size_t g = 0; g < p.groups.size(); ++g) {
        const Group& gr = p.groups[g];
        CHECK(b.owner.count(gr.block) && b.owner.at(gr.block) == gr.owner && p.group.at(gr.block) == g);
        CHECK(g == 0 || gr.owner > last_owner); // in order of first touch
        last_owner = gr.owner;
        const auto& w = b.writer.at(gr.block);
        uint32_t lo = 0, hi = (uint32_t)ds;
        while (lo < ds && w[lo] == -1)
            ++lo;
        while (hi > 0 && w[hi - 1] == -1)
            --hi;
        CHECK(gr.lo == lo && gr.hi == hi && lo < hi && hi <= ds);
    }
    for (auto& [number, entry] : b.winner)
        CHECK(p.winner.count(number) && p.winner.at(number) == entry);
    if (g_fail)
        std::printf("  in case %s, ds %llu, seed %u\n", what, (unsigned long long)ds, seed);
}

static void test_row()
{
    Inode in;
    uint8_t* raw = (uint8_t*)&in;
    for (uint32_t i = 0; i < 81; ++i)
        raw[i] = (uint8_t)(37u * i + 11u);
    uint8_t file[64];
    std::memcpy(file, raw + 16, 64);
    std::vector<uint8_t> row(81); // exactly 81 bytes on the heap
    for (uint32_t i = 0; i < 81; ++i)
        row[i] = (uint8_t)row_byte(in.time_creation, in.time_modified, in.type, [&](uint32_t b) -> uint32_t { return file[b]; }, i);
    CHECK(std::memcmp(row.data(), raw, 81) == 0);
    CHECK(offsetof(Inode, direct) == FILE_OFF && offsetof(Inode, type) == TYPE_OFF && offsetof(Inode, file_size) == 76);
}

int main()
{
    test_row();
    CHECK(capacity(0) == 2 && capacity(1) == 2 && capacity(2) == 4 && capacity(3) == 8 && capacity(32768) == 65536);
    for (uint64_t ds : { 1ull, 31ull, 79ull, 80ull, 81ull, 249ull, 4091ull }) {
        const uint32_t m = (uint32_t)piece_inodes(ds);
        std::mt19937 rng((uint32_t)ds);
        // a full piece of distinct numbers, one in ten not taking part
        std::vector<uint32_t> pool(3 * m), ino, verdict(m, 0);
        for (uint32_t i = 0; i < pool.size(); ++i)
            pool[i] = i;
        std::shuffle(pool.begin(), pool.end(), rng);
        ino.assign(pool.begin(), pool.begin() + m);
        for (uint32_t j = 0; j < m; ++j)
            verdict[j] = rng() % 10 == 0 ? (rng() % 2 ? 255u : 9u) : 0u;
        for (uint32_t seed = 1; seed <= 3; ++seed)
            run_case("distinct", ds, 7, ino, verdict, seed);
        // the maximal load: a full piece of distinct, consecutive numbers, all taking part
        std::vector<uint32_t> all(m, 0);
        for (uint32_t j = 0; j < m; ++j)
            ino[j] = 1000 + j;
        run_case("consecutive", ds, 7, ino, all, 4);
        // a full piece of one repeated number
        std::fill(ino.begin(), ino.end(), 12345u);
        run_case("one number", ds, 7, ino, all, 5);
        // repeats among distinct numbers, a table that ends past block 2^32 - 2
        for (uint32_t j = 0; j < m; ++j)
            ino[j] = rng() % (m / 3 + 1);
        run_case("repeats", ds, 7, ino, verdict, 6);
        run_case("past the last block", ds, 0xFFFFFFFFu - 40u, ino, verdict, 7);
    }
    std::printf("longest probe sequence: %u\n", g_max_steps);
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
