// test_file_plan.cpp -- csrc/file_plan.hpp (the arithmetic of the read-only file walk) against naive
// restatements of FileIO's BlockIndexIterator (file_io.cpp:186-463) and FileIO::readFile (:12-44).  A plain
// host program: built with g++ -fsanitize=address,undefined by tests/test_file_cpu.py; the expansion runs
// over heap buffers of exactly the scratch's size, so a read past a payload's end is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "../../paritypartyfs_amd/csrc/extent_plan.hpp"
#include "../../paritypartyfs_amd/csrc/file_plan.hpp"

using namespace ppfs::fileplan;

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

// The iterator, one step at a time: counters per level that carry like the reference's
struct Naive {
    uint64_t I;
    uint32_t segment = 0;
    uint64_t a = 0, b = 0, c = 0; // slots, outermost first
    void next()
    {
        if (segment == 0) {
            if (++a == DIRECT) {
                segment = I ? 1 : 4;
                a = 0;
            }
        } else if (segment == 1) {
            if (++a == I) {
                segment = 2;
                a = 0;
            }
        } else if (segment == 2) {
            if (++b == I) {
                b = 0;
                if (++a == I) {
                    segment = 3;
                    a = 0;
                }
            }
        } else if (segment == 3) {
            if (++c == I) {
                c = 0;
                if (++b == I) {
                    b = 0;
                    if (++a == I)
                        segment = 4;
                }
            }
        }
    }
};

static void test_path_of()
{
    for (uint64_t I : { (uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)14, (uint64_t)62 }) {
        const uint64_t cap = capacity_ipb(I);
        CHECK(cap == 12 + I + I * I + I * I * I, "I %llu", (unsigned long long)I);
        Naive it { I };
        for (uint64_t j = 0; j < cap + 3; ++j, it.next()) {
            const Path p = path_of(j, I);
            CHECK(p.segment == it.segment, "I %llu j %llu segment %u vs %u", (unsigned long long)I, (unsigned long long)j, p.segment,
                it.segment);
            if (it.segment == 4) {
                CHECK(j >= cap, "past capacity");
                continue;
            }
            CHECK(j < cap && p.depth == p.segment, "depth");
            CHECK(p.slot[0] == it.a && (p.segment < 2 || p.slot[1] == it.b) && (p.segment < 3 || p.slot[2] == it.c),
                "I %llu j %llu slots", (unsigned long long)I, (unsigned long long)j);
        }
    }
    CHECK(capacity(3) == 12 && capacity(0) == 12 && capacity(4) == 15 && capacity(58) == 12 + 14 + 196 + 2744, "capacity(ds)");
    CHECK(capacity(65535) == (uint64_t)12 + (uint64_t)16383 + (uint64_t)16383 * (uint64_t)16383 + (uint64_t)16383 * (uint64_t)16383 * (uint64_t)16383, "64-bit capacity");
    CHECK(occupied(0, 58) == 0 && occupied(1, 58) == 1 && occupied(58, 58) == 1 && occupied(59, 58) == 2 && occupied(5, 0) == 0,
        "occupied");
}

using Id = std::tuple<int, long long, long long>; // segment, outer slot, inner slot (-1: none)

static void test_trees()
{
    for (uint64_t I : { (uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3 }) {
        const uint64_t cap = capacity_ipb(I);
        for (uint64_t j0 = 0; j0 <= cap; ++j0)
            for (uint64_t count = 0; j0 + count <= cap; ++count) {
                // brute force: the index blocks in the order the walk first needs them, per level
                std::vector<Id> lv[3];
                std::map<Id, uint64_t> first;
                auto need = [&](int level, Id id, uint64_t j) {
                    if (!first.count(id)) {
                        first[id] = j;
                        lv[level].push_back(id);
                    }
                };
                for (uint64_t j = j0; j < j0 + count; ++j) {
                    const Path p = path_of(j, I);
                    if (p.segment >= 1)
                        need(0, Id { (int)p.segment, -1, -1 }, j);
                    if (p.segment >= 2)
                        need(1, Id { (int)p.segment, (long long)p.slot[0], -1 }, j);
                    if (p.segment == 3)
                        need(2, Id { 3, (long long)p.slot[0], (long long)p.slot[1] }, j);
                }
                const Tree t = tree_of(j0, count, I);
                CHECK(t.nA == lv[0].size() && t.nB == lv[1].size() && t.nC == lv[2].size(), "I %llu j0 %llu n %llu counts",
                    (unsigned long long)I, (unsigned long long)j0, (unsigned long long)count);
                if (t.nA != lv[0].size() || t.nB != lv[1].size() || t.nC != lv[2].size())
                    continue;
                CHECK(tree_blocks(t) == first.size() && level_count(t, LEVEL_DATA) == count, "totals");
                CHECK(entry_base(t, LEVEL_A) == 0 && entry_base(t, LEVEL_B) == t.nA && entry_base(t, LEVEL_C) == t.nA + t.nB, "entry bases");
                CHECK(slot_base(t, LEVEL_B) % 16 == 0 && slot_base(t, LEVEL_B) >= t.nA && slot_base(t, LEVEL_C) % 16 == 0
                        && slot_base(t, LEVEL_C) >= slot_base(t, LEVEL_B) + t.nB && tree_slots(t) == slot_base(t, LEVEL_C) + t.nC,
                    "slot bases");
                auto find = [&](int level, Id id) -> long long {
                    for (size_t k = 0; k < lv[level].size(); ++k)
                        if (lv[level][k] == id)
                            return (long long)k;
                    return -1;
                };
                for (int level = 0; level < 3; ++level)
                    for (uint64_t k = 0; k < lv[level].size(); ++k) {
                        const Id id = lv[level][k];
                        const Ref r = ref_of(t, level, k);
                        CHECK(first_under(t, level, k) == first[id], "I %llu j0 %llu n %llu level %d k %llu first %llu vs %llu",
                            (unsigned long long)I, (unsigned long long)j0, (unsigned long long)count, level, (unsigned long long)k,
                            (unsigned long long)first_under(t, level, k), (unsigned long long)first[id]);
                        if (level == 0) {
                            CHECK(r.level == LEVEL_INODE && r.slot == 11u + (uint32_t)std::get<0>(id), "root dword");
                        } else if (level == 1) {
                            CHECK(r.level == LEVEL_A && (long long)r.parent_k == find(0, Id { std::get<0>(id), -1, -1 })
                                    && r.slot == (uint32_t)std::get<1>(id),
                                "level B parent");
                        } else {
                            CHECK(r.level == LEVEL_B && (long long)r.parent_k == find(1, Id { 3, std::get<1>(id), -1 })
                                    && r.slot == (uint32_t)std::get<2>(id),
                                "level C parent");
                        }
                    }
                for (uint64_t k = 0; k < count; ++k) {
                    const Path p = path_of(j0 + k, I);
                    const Ref r = ref_of(t, LEVEL_DATA, k);
                    bool ok = false;
                    if (p.segment == 0)
                        ok = r.level == LEVEL_INODE && r.slot == p.slot[0];
                    else if (p.segment == 1)
                        ok = r.level == LEVEL_A && (long long)r.parent_k == find(0, Id { 1, -1, -1 }) && r.slot == p.slot[0];
                    else if (p.segment == 2)
                        ok = r.level == LEVEL_B && (long long)r.parent_k == find(1, Id { 2, (long long)p.slot[0], -1 }) && r.slot == p.slot[1];
                    else
                        ok = r.level == LEVEL_C && (long long)r.parent_k == find(2, Id { 3, (long long)p.slot[0], (long long)p.slot[1] })
                            && r.slot == p.slot[2];
                    CHECK(ok, "I %llu j0 %llu n %llu data k %llu", (unsigned long long)I, (unsigned long long)j0, (unsigned long long)count,
                        (unsigned long long)k);
                }
            }
    }
}

// span and the closed-form extents against FileIO::readFile's loop (extent_plan.hpp file_extents)
static void test_span()
{
    for (uint64_t ds : { (uint64_t)1, (uint64_t)3, (uint64_t)4, (uint64_t)58, (uint64_t)99, (uint64_t)249 })
        for (uint64_t fs : { (uint64_t)0, (uint64_t)1, ds - 1, ds, ds + 1, 5 * ds, 5 * ds + 7, 40 * ds - 1 })
            for (uint64_t offset = 0; offset <= fs + 2; offset += (offset < 3 * ds + 2 ? 1 : ds / 2 + 1))
                for (uint64_t nb : { (uint64_t)0, (uint64_t)1, (uint64_t)2, ds - 1, ds, ds + 1, 3 * ds, 3 * ds + 5, fs, fs + 9, (uint64_t)1 << 40 }) {
                    const Span sp = span(fs, ds, offset, nb);
                    if (nb == 0) {
                        CHECK(sp.ok && sp.count == 0 && sp.bytes == 0, "empty range");
                        continue;
                    }
                    if (offset >= fs) {
                        CHECK(!sp.ok, "offset at or past the end");
                        continue;
                    }
                    const uint64_t bytes = std::min(nb, fs - offset), last = (offset + bytes - 1) / ds;
                    CHECK(sp.ok && sp.bytes == bytes && sp.first == offset / ds && sp.count == last - offset / ds + 1,
                        "ds %llu fs %llu off %llu n %llu", (unsigned long long)ds, (unsigned long long)fs, (unsigned long long)offset,
                        (unsigned long long)nb);
                    CHECK(sp.first + sp.count <= occupied(fs, ds), "inside the file");
                    std::vector<uint32_t> idx(sp.count + 2);
                    for (size_t i = 0; i < idx.size(); ++i)
                        idx[i] = 1000u + (uint32_t)i;
                    std::vector<ppfs_ecc_extent> ref;
                    const size_t done = ppfs::extplan::file_extents(idx.data(), idx.size(), offset % ds, bytes, ds, ref);
                    CHECK(done == bytes && ref.size() == sp.count, "file_extents covers the range with span's blocks");
                    for (size_t i = 0; i < ref.size() && i < sp.count; ++i) {
                        const Extent x = extent_of(i, offset % ds, bytes, ds);
                        CHECK(x.pos == ref[i].pos && x.offset == ref[i].offset && x.length == ref[i].length && x.length > 0,
                            "ds %llu off %llu n %llu extent %zu", (unsigned long long)ds, (unsigned long long)offset, (unsigned long long)nb, i);
                    }
                }
    CHECK(!span(10, 0, 0, 1).ok, "no payload, no file");
}

// expand over a model tree: every index block is a vector of entries; statuses 1 / 5 / 9 in turn
struct Src {
    const uint32_t* file;
    const uint8_t *payload, *st, *inh;
    uint32_t inode(uint32_t dw) const { return file[dw]; }
    uint32_t status(uint64_t p) const { return st[p]; }
    uint32_t inherited(uint64_t p) const { return inh[p]; }
    uint32_t payload_byte(uint64_t at) const { return payload[at]; }
};

static void test_expand()
{
    uint32_t seed = 12345;
    auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u; };
    for (uint64_t ds : { (uint64_t)4, (uint64_t)9, (uint64_t)12, (uint64_t)15 }) {
        const uint64_t I = ipb_of(ds), cap = capacity_ipb(I);
        // the model: a fresh block number for every node, entries by identity
        std::map<Id, uint32_t> blockno;
        uint32_t next_block = 100;
        auto block_of = [&](Id id) {
            if (!blockno.count(id))
                blockno[id] = next_block += 1 + rnd() % 7;
            return blockno[id];
        };
        auto data_block = [&](uint64_t j) { return 5000u + (uint32_t)j * 3u; };
        uint32_t file[16];
        for (int d = 0; d < 12; ++d)
            file[d] = data_block(d);
        file[12] = block_of(Id { 1, -1, -1 });
        file[13] = block_of(Id { 2, -1, -1 });
        file[14] = block_of(Id { 3, -1, -1 });
        file[15] = 0;
        // entry `slot` of node id
        auto entry = [&](Id id, uint64_t slot) -> uint32_t {
            const int seg = std::get<0>(id);
            const long long a = std::get<1>(id), b = std::get<2>(id);
            if (seg == 1)
                return data_block(12 + slot);
            if (seg == 2)
                return a < 0 ? block_of(Id { 2, (long long)slot, -1 }) : data_block(12 + I + a * I + slot);
            if (a < 0)
                return block_of(Id { 3, (long long)slot, -1 });
            if (b < 0)
                return block_of(Id { 3, a, (long long)slot });
            return data_block(12 + I + I * I + (a * I + b) * I + slot);
        };
        for (int bad_level = -1; bad_level < 3; ++bad_level)
            for (uint32_t bad : { 5u, 9u, 1u })
                for (uint64_t j0 : { (uint64_t)0, (uint64_t)5, (uint64_t)12, cap / 2, cap - 1 })
                    for (uint64_t count : { (uint64_t)1, (uint64_t)9, cap - j0 }) {
                        if (j0 + count > cap || (bad_level < 0 && bad != 5u))
                            continue;
                        const Tree t = tree_of(j0, count, I);
                        const uint64_t slots = tree_slots(t);
                        std::vector<uint8_t> payload(slots * ds, 0xEE), st(slots, 0), inh(slots, 0);
                        std::vector<Id> ids(slots, Id { 0, 0, 0 });
                        std::vector<uint32_t> tidx(slots, 0);
                        const Src src { file, payload.data(), st.data(), inh.data() };
                        for (int level = 0; level < 3; ++level) {
                            const uint64_t n = level_count(t, level), at = slot_base(t, level);
                            const uint64_t bad_k = n ? rnd() % n : 0;
                            for (uint64_t k = 0; k < n; ++k) {
                                const Ref r = ref_of(t, level, k);
                                const Expanded e = expand(t, level, k, ds, src);
                                Id id;
                                if (level == 0)
                                    id = Id { (int)r.slot - 11, -1, -1 };
                                else {
                                    const Id pid = ids[slot_base(t, r.level) + r.parent_k];
                                    id = level == 1 ? Id { std::get<0>(pid), (long long)r.slot, -1 } : Id { 3, std::get<1>(pid), (long long)r.slot };
                                }
                                ids[at + k] = id;
                                tidx[at + k] = e.pointer;
                                inh[at + k] = e.inherited;
                                if (e.inherited) {
                                    CHECK(e.pointer == NO_BLOCK, "a failed path has no pointer");
                                    st[at + k] = 9; // what the list decode gives NO_BLOCK
                                    continue;
                                }
                                CHECK(e.pointer == block_of(id), "ds %llu level %d k %llu pointer", (unsigned long long)ds, level,
                                    (unsigned long long)k);
                                st[at + k] = level == bad_level && k == bad_k ? (uint8_t)bad : 0;
                                if (st[at + k] == 5 || st[at + k] == 9)
                                    continue; // payload undefined: stays 0xEE
                                for (uint64_t sl = 0; sl < I; ++sl) {
                                    const uint32_t v = entry(id, sl);
                                    for (int q = 0; q < 4; ++q)
                                        payload[(at + k) * ds + 4 * sl + q] = (uint8_t)(v >> (8 * q));
                                }
                            }
                        }
                        for (uint64_t k = 0; k < count; ++k) {
                            const uint64_t j = j0 + k;
                            const Path p = path_of(j, I);
                            const Expanded e = expand(t, LEVEL_DATA, k, ds, src);
                            // the expected path status: the first failed node from the root down
                            uint32_t want = 0;
                            for (uint64_t s = 0; s < slots && !want; ++s) {
                                if (st[s] != 5 && st[s] != 9)
                                    continue;
                                if (inh[s])
                                    continue;
                                const Id id = ids[s];
                                const bool above = std::get<0>(id) == (int)p.segment
                                    && (std::get<1>(id) < 0 || (std::get<1>(id) == (long long)p.slot[0]
                                           && (p.segment == 2 || std::get<2>(id) < 0 || std::get<2>(id) == (long long)p.slot[1])));
                                bool used = false; // is s a live slot of the tree?
                                for (int level = 0; level < 3; ++level)
                                    used |= s >= slot_base(t, level) && s < slot_base(t, level) + level_count(t, level);
                                if (above && used)
                                    want = st[s];
                            }
                            CHECK(e.inherited == want, "ds %llu j %llu path status %u vs %u", (unsigned long long)ds, (unsigned long long)j,
                                e.inherited, want);
                            CHECK(e.pointer == (want ? NO_BLOCK : data_block(j)), "ds %llu j %llu data pointer", (unsigned long long)ds,
                                (unsigned long long)j);
                        }
                    }
    }
}

int main()
{
    test_path_of();
    test_trees();
    test_span();
    test_expand();
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
