#pragma once
// inode_wplan.hpp -- the grouping step of the inode writes (inode_path.cpp ppfs_ecc_write_inodes_*, inode_walk.hip):
// from "many byte ranges, several per table block" to "one row per distinct block, all its ranges overlaid".  For
// host and device alike: the kernels, the host form and tests/cpp/test_inode_wplan.cpp run the same insert and lookup
// code, the test serially in shuffled orders under the sanitizers.
//
// InodeManager::update (lib/inode_manager/src/inode_manager.cpp:142-159) is Bitmap::getBit and _writeInode (:20-54),
// one writeBlock per piece of the 81 bytes (inode_plan.hpp piece()).  A piece of a batch is m inodes of K = K(ds)
// slots each, slot = j * K + k for piece k of entry j; a slot TAKES PART as inode_plan.hpp slot_of says, which the
// reads' table extents use too.  This file is the election only.
//   elect    two open-addressing tables of `cap` = capacity(m * K) entries, keys and values 32-bit, all 0xFF when
//            cleared.  blocks: key = block number, value = the LOWEST slot that touches it (unsigned minimum): the
//            block's owner, whose slot index is the block's row in the extent staging.  inodes: key = inode number,
//            value = the HIGHEST entry that names it (signed maximum; cleared = -1): the winner among repeats, as the
//            loop's later update overwrites the earlier one.  Linear probing; a probe loop ends after at most cap
//            steps, a lane never waits for another one.  Keys are claimed by compare-and-swap and never change again,
//            so a lookup after the elect pass needs no atomics.
//   extents  the owner slot of a block emits {pos 0, block, offset 0, length 0}: the extent write checks the old
//            block, hands its payload to the overlay and encodes it again; every other slot emits the invalid extent.
//   overlay  a slot that takes part and whose entry is its inode's winner stores its `length` bytes of the composed
//            row at payload row owner(block), byte offset.  Distinct inodes do not overlap and repeats have one
//            winner: every payload byte has one writer.
//   merge    a slot's write status is its owner's, a 1 turned into 0 for every slot but the owner (the first toucher
//            reports the correction, as in the loop); then inode_plan.hpp table_status.
// The host form needs no tables: plan_host() groups with an ordinary map and gives, per distinct block, the owner slot
// and the hull [lo, hi) of the batch's bytes in it, which is what one ppfs_ecc_write_extents_host entry covers.
#include <stdint.h>

#include "inode_plan.hpp"

#include <unordered_map>
#include <vector>

namespace ppfs {
namespace inodewplan {

using namespace inodeplan;

constexpr uint32_t EMPTY = 0xFFFFFFFFu; // a cleared key or value; no block (NO_BLOCK) and no inode number (< total_inodes)

// a power of two, at least twice the slots and at least 2
PPFS_HD inline uint32_t capacity(uint64_t slots)
{
    uint32_t cap = 2;
    while ((uint64_t)cap < 2u * slots && cap < 0x80000000u)
        cap <<= 1;
    return cap;
}
// bytes of the two tables: block keys, block values, inode keys, inode values
PPFS_HD inline uint64_t table_bytes(uint32_t cap) { return 16ull * cap; }

// Fibonacci hashing: consecutive block and inode numbers, the usual batch, spread evenly.  cap: a power of two >= 2
PPFS_HD inline uint32_t home(uint32_t key, uint32_t cap)
{
    return (key * 2654435769u) >> (uint32_t)(__builtin_clz(cap) + 1); // 32 - log2(cap)
}

// the host's memory operations, one caller at a time; inode_walk.hip has the device's, atomics with the same meaning
struct SerialOps {
    static uint32_t load(const uint32_t* a, uint32_t i, uint32_t) { return a[i]; }
    static uint32_t cas(uint32_t* a, uint32_t i, uint32_t, uint32_t expect, uint32_t v)
    {
        const uint32_t old = a[i];
        if (old == expect)
            a[i] = v;
        return old;
    }
    static void min_u32(uint32_t* a, uint32_t i, uint32_t, uint32_t v)
    {
        if (v < a[i])
            a[i] = v;
    }
    static void max_i32(uint32_t* a, uint32_t i, uint32_t, uint32_t v)
    {
        if ((int32_t)v > (int32_t)a[i])
            a[i] = v;
    }
};

// The place of `key` in keys[cap], claimed if it was not there; EMPTY when cap probes found neither the key nor a free
// place (impossible at the load the capacity allows).  steps (may be null): the probes made.
template <class Ops>
PPFS_HD inline uint32_t claim(uint32_t* keys, uint32_t cap, uint32_t key, uint32_t* steps = nullptr)
{
    uint32_t h = home(key, cap);
    for (uint32_t i = 0; i < cap; ++i, h = (h + 1u) & (cap - 1u)) {
        const uint32_t old = Ops::cas(keys, h, cap, EMPTY, key);
        if (old == EMPTY || old == key) {
            if (steps)
                *steps = i + 1u;
            return h;
        }
    }
    if (steps)
        *steps = cap;
    return EMPTY;
}
// The place of `key`, EMPTY when it is not in the table.  After the elect pass: plain loads.
template <class Ops>
PPFS_HD inline uint32_t find(const uint32_t* keys, uint32_t cap, uint32_t key)
{
    uint32_t h = home(key, cap);
    for (uint32_t i = 0; i < cap; ++i, h = (h + 1u) & (cap - 1u)) {
        const uint32_t k = Ops::load(keys, h, cap);
        if (k == key)
            return h;
        if (k == EMPTY)
            return EMPTY;
    }
    return EMPTY;
}

// the two tables in one cleared allocation of table_bytes(cap)
struct Tables {
    uint32_t *bkey, *bval, *ikey, *ival;
    uint32_t cap;
};
PPFS_HD inline Tables tables_at(uint32_t* base, uint32_t cap) { return Tables { base, base + cap, base + 2ull * cap, base + 3ull * cap, cap }; }

// elect: slot `slot` = entry j, piece k; s: inode_plan.hpp slot_of
template <class Ops>
PPFS_HD inline void elect(const Tables& t, const Slot& s, uint32_t ino, uint32_t j, uint32_t k, uint32_t slot)
{
    if (!s.takes_part)
        return;
    const uint32_t b = claim<Ops>(t.bkey, t.cap, s.block);
    if (b != EMPTY)
        Ops::min_u32(t.bval, b, t.cap, slot);
    if (k == 0u) {
        const uint32_t i = claim<Ops>(t.ikey, t.cap, ino);
        if (i != EMPTY)
            Ops::max_i32(t.ival, i, t.cap, j);
    }
}
// the owner slot of a block, the winning entry of an inode number; EMPTY when the key was never elected
template <class Ops>
PPFS_HD inline uint32_t owner_of(const Tables& t, uint32_t block)
{
    const uint32_t b = find<Ops>(t.bkey, t.cap, block);
    return b == EMPTY ? EMPTY : Ops::load(t.bval, b, t.cap);
}
template <class Ops>
PPFS_HD inline uint32_t winner_of(const Tables& t, uint32_t ino)
{
    const uint32_t i = find<Ops>(t.ikey, t.cap, ino);
    return i == EMPTY ? EMPTY : Ops::load(t.ival, i, t.cap);
}

// Byte i < 81 of the packed Inode (inode.hpp:18-41) that an entry writes: time_creation, time_modified, the 64 bytes
// of its ppfs_ecc_file record, type.  file(b): byte b < 64 of the record.
template <class FileByte>
PPFS_HD inline uint32_t row_byte(uint64_t time_creation, uint64_t time_modified, uint32_t type, FileByte file, uint32_t i)
{
    if (i < 8u)
        return (uint32_t)(time_creation >> (8u * i)) & 0xFFu;
    if (i < FILE_OFF)
        return (uint32_t)(time_modified >> (8u * (i - 8u))) & 0xFFu;
    if (i < TYPE_OFF)
        return (uint32_t)file(i - FILE_OFF) & 0xFFu;
    return type & 0xFFu;
}

// The status piece `slot` reports for the write status `wst` of its block's owner row: the first toucher rule
PPFS_HD inline uint32_t seen_status(uint32_t wst, uint32_t slot, uint32_t owner) { return wst == ST_CORRECTED && slot != owner ? ST_OK : wst; }

// ---- the host form's plan (host code only) ----
struct Group {
    uint32_t block, owner; // the lowest slot that touches the block
    uint32_t lo, hi;       // the hull of the batch's bytes in the block
};
struct HostPlan {
    std::vector<Group> groups;                     // in order of first touch
    std::unordered_map<uint32_t, uint32_t> group;  // block -> index into groups
    std::unordered_map<uint32_t, uint32_t> winner; // inode number -> its highest entry
};
// verdict[j]: inode_plan.hpp bitmap_verdict of entry j
inline HostPlan plan_host(const uint32_t* ino, const uint32_t* verdict, uint64_t n, uint32_t table_block, uint64_t ds)
{
    HostPlan p;
    const uint32_t K = max_pieces(ds);
    for (uint64_t j = 0; j < n; ++j) {
        for (uint32_t k = 0; k < K; ++k) {
            const Slot s = slot_of(table_block, ino[j], k, verdict[j], ds);
            if (!s.takes_part)
                continue;
            auto it = p.group.find(s.block);
            if (it == p.group.end()) {
                p.group.emplace(s.block, (uint32_t)p.groups.size());
                p.groups.push_back(Group { s.block, (uint32_t)(j * K + k), s.offset, s.offset + s.length });
            } else {
                Group& g = p.groups[it->second];
                g.lo = s.offset < g.lo ? s.offset : g.lo;
                g.hi = s.offset + s.length > g.hi ? s.offset + s.length : g.hi;
            }
            if (k == 0u)
                p.winner[ino[j]] = (uint32_t)j;
        }
    }
    return p;
}

} // namespace inodewplan
} // namespace ppfs
