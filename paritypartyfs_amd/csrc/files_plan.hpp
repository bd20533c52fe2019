#pragma once
// files_plan.hpp -- the arithmetic of a walk over a BATCH of files, a batch of one included (files_path.cpp,
// files_walk.hip): the single-file plan of file_plan.hpp applied to file after file, with every level of
// all the files merged into one list, so that a batch costs the launches of one file.  Plain arithmetic for host and device
// alike; tests/cpp/test_files_plan.cpp (a plain g++ program under the address sanitizer) checks it against
// a per-file loop of file_plan.hpp.
//
// Range f of a batch is readFile(offset, nbytes) of file f: fileplan::span gives its first file block, its
// blocks and its clamped bytes.  The batch's arrays hold the files back to back, in batch order:
//   per-block arrays (index, path status, status)   file f at [block_pos, block_pos + blocks)
//   out                                              file f at [out_pos, out_pos + bytes), no padding
//   tree arrays (tree_index, tree_status)            LEVEL-MAJOR: level A of every file, then level B of
//                                                    every file, then level C; file f's level l at
//                                                    [tree_pos[l], tree_pos[l] + tree_n[l]); within one
//                                                    file's level the order is file_plan.hpp's
// In the scratch of a call the three merged levels start on 16-entry boundaries (Levels), which is the
// single-file rule: every level's payload and status pointers keep the list decode's 16-byte rule.  A
// file's entries are contiguous within a level; there is no per-file alignment, so merged entry e of level
// l lies in scratch slot base[l] + e.
//
// Which file owns merged entry e of a level has no closed form.  Per level (A, B, C, data) a table of Rows
// (first entry, file number) lists the files that have at least one entry there, ascending, plus a sentinel
// (the level's total, nfiles); row_of is upper_bound - 1.  Files without entries at a level never appear, so
// rows start at distinct entries and 256 consecutive entries span at most 256 rows.  What a kernel needs of
// the owning file is its FileRec, 128 bytes.
#include <stdint.h>

#include "file_plan.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

namespace ppfs {
namespace filesplan {

constexpr int LEVELS = 4; // fileplan::LEVEL_A, LEVEL_B, LEVEL_C, LEVEL_DATA index the row tables
// the file flags: bits 0-2 from a file's data blocks, the same three from bit 8 for its index blocks
constexpr uint32_t FLAG_CORRECTED = 1u, FLAG_FAILED = 2u, FLAG_OUT = 4u, FLAG_TREE_SHIFT = 8u;
PPFS_HD inline uint32_t flag_of(uint32_t status)
{
    return status == 1u ? FLAG_CORRECTED : status == fileplan::STATUS_FAILED ? FLAG_FAILED
        : status == fileplan::STATUS_OUT                                     ? FLAG_OUT
                                                                             : 0u;
}

// where file f's results lie in the batch's arrays (the ABI's ppfs_ecc_files_slot, field for field)
struct Slot {
    uint64_t first, blocks, bytes; // fileplan::span of its range
    uint64_t block_pos, out_pos;
    uint64_t tree_pos[3], tree_n[3];
};
// the batch's sizes, also the running sums while a plan is built (ppfs_ecc_files_totals)
struct Totals {
    uint64_t blocks, bytes, tree[3], tree_blocks;
};
// where the merged levels start in a call's scratch, and its slots in all
struct Levels {
    uint64_t base[3], slots;
};
PPFS_HD inline Levels levels_of(const Totals& t)
{
    Levels l;
    l.base[0] = 0;
    l.base[1] = fileplan::round16(t.tree[0]);
    l.base[2] = l.base[1] + fileplan::round16(t.tree[1]);
    l.slots = t.tree_blocks ? l.base[2] + t.tree[2] : 0u;
    return l;
}

enum Bad : int { RANGE_OK = 0, BAD_OFFSET = 1, BAD_CAPACITY = 2 };
// The slot of the next file of a batch whose files so far add up to `sum`; tree_pos[l] counts within level l
// (level_major turns the positions into the level-major ones once the totals are known).
PPFS_HD inline int next_slot(uint64_t file_size, uint64_t ds, uint64_t offset, uint64_t nbytes, const Totals& sum, Slot& s)
{
    const fileplan::Span sp = fileplan::span(file_size, ds, offset, nbytes);
    if (!sp.ok)
        return BAD_OFFSET;
    if (sp.first + sp.count > fileplan::capacity(ds))
        return BAD_CAPACITY;
    const fileplan::Tree t = fileplan::tree_of(sp.first, sp.count, fileplan::ipb_of(ds));
    s.first = sp.first;
    s.blocks = sp.count;
    s.bytes = sp.bytes;
    s.block_pos = sum.blocks;
    s.out_pos = sum.bytes;
    for (int l = 0; l < 3; ++l) {
        s.tree_pos[l] = sum.tree[l];
        s.tree_n[l] = fileplan::level_count(t, l);
    }
    return RANGE_OK;
}
PPFS_HD inline void add_slot(Totals& sum, const Slot& s)
{
    sum.blocks += s.blocks;
    sum.bytes += s.bytes;
    for (int l = 0; l < 3; ++l) {
        sum.tree[l] += s.tree_n[l];
        sum.tree_blocks += s.tree_n[l];
    }
}
PPFS_HD inline void level_major(Slot& s, const Totals& total)
{
    s.tree_pos[1] += total.tree[0];
    s.tree_pos[2] += total.tree[0] + total.tree[1];
}

// a row of a level's table: the file whose entries start at merged entry `first`
struct Row {
    uint64_t first;
    uint32_t file, pad;
};
// the row that owns entry i: the last one whose first <= i.  rows >= 1, table[0].first == 0 (the sentinel
// table[rows] is not read)
PPFS_HD inline uint64_t row_of(const Row* table, uint64_t rows, uint64_t i)
{
    uint64_t lo = 0, hi = rows;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (table[mid].first <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// what the kernels need of one file: 128 bytes
struct FileRec {
    uint32_t inode[16];      // the record as sixteen dwords
    uint64_t first, blocks;  // its range's file blocks; the Tree is rebuilt from them (tree_of)
    uint64_t off0, bytes;    // offset % ds and the clamped bytes
    uint64_t out_pos;
    uint64_t lvl[3];         // where its levels A, B, C start in the scratch
};
static_assert(sizeof(Row) == 16 && sizeof(FileRec) == 128, "table rows are 16 bytes, file records 128");

// Mem: status(p) / inherited(p) / payload_byte(at) of the merged scratch, as fileplan::expand's Src
template <class Mem>
struct RecSrc {
    const FileRec* rec;
    const Mem* mem;
    PPFS_HD uint32_t inode(uint32_t dw) const { return dw < 16u ? rec->inode[dw] : fileplan::NO_BLOCK; }
    PPFS_HD uint32_t status(uint64_t p) const { return mem->status(p); }
    PPFS_HD uint32_t inherited(uint64_t p) const { return mem->inherited(p); }
    PPFS_HD uint32_t payload_byte(uint64_t at) const { return mem->payload_byte(at); }
};
// entry k of a level of the file of `rec`: fileplan's expansion against the merged scratch.  A k past the
// level (a table that does not go with the records) names no block.
// t: the Tree of the record's range, for a caller that has it already
template <class Mem>
PPFS_HD inline fileplan::Expanded expand_entry(const FileRec& rec, const fileplan::Tree& t, int level, uint64_t k, uint64_t ds,
    const Mem& mem)
{
    if (k >= fileplan::level_count(t, level))
        return fileplan::Expanded { fileplan::NO_BLOCK, fileplan::STATUS_OUT };
    const RecSrc<Mem> src { &rec, &mem };
    return fileplan::expand_at(t, level, k, ds, src, rec.lvl[0], rec.lvl[1], rec.lvl[2]);
}
template <class Mem>
PPFS_HD inline fileplan::Expanded expand_entry(const FileRec& rec, int level, uint64_t k, uint64_t ds, const Mem& mem)
{
    return expand_entry(rec, fileplan::tree_of(rec.first, rec.blocks, fileplan::ipb_of(ds)), level, k, ds, mem);
}

// The host-built plan of a batch.  rows[l] ends with the sentinel, so rows[l].size() - 1 files have entries
// at level l (an empty level holds the sentinel alone).
struct Plan {
    std::vector<Slot> slots;
    std::vector<FileRec> recs;
    std::vector<Row> rows[LEVELS];
    Totals total {};
    Levels levels {};
    uint64_t count(int level) const { return level < 3 ? total.tree[level] : total.blocks; }
    struct PlanView view() const;
};
// What a walk reads of a plan, a batch's (Plan::view) or a single file's (OnePlan::view): pointers into the plan, which
// outlives the view.  rows[l] holds nrows[l] rows and then the sentinel.  one: a single file's record with its Tree
// (recs then points at its record); null for a batch.
struct OneRec;
struct PlanView {
    const FileRec* recs;
    uint64_t nfiles;
    const Row* rows[LEVELS];
    uint64_t nrows[LEVELS];
    Totals total;
    Levels levels;
    const OneRec* one = nullptr;
};
inline PlanView Plan::view() const
{
    PlanView v { recs.data(), recs.size(), {}, {}, total, levels };
    for (int l = 0; l < LEVELS; ++l) {
        v.rows[l] = rows[l].data();
        v.nrows[l] = rows[l].size() - 1;
    }
    return v;
}
// the record of a file out of its inode, its slot (tree_pos still counted within each level) and the merged levels
inline FileRec rec_of(const uint32_t* inode, const Slot& s, uint64_t off0, const Levels& levels)
{
    FileRec q;
    for (int d = 0; d < 16; ++d)
        q.inode[d] = inode[d];
    q.first = s.first;
    q.blocks = s.blocks;
    q.off0 = s.blocks ? off0 : 0u;
    q.bytes = s.bytes;
    q.out_pos = s.out_pos;
    for (int l = 0; l < 3; ++l)
        q.lvl[l] = levels.base[l] + s.tree_pos[l];
    return q;
}
// The range rule of a WRITE (ppfs_ecc_write_file_*, ppfs_ecc_write_files_*): it stays inside the file as the inode
// describes it, offset + nbytes <= file_size, and nothing is clamped (FileIO::writeFile would grow the file,
// file_io.cpp:46-104; growing is the caller's job).  nbytes == 0 is an empty, valid range whatever the offset.
constexpr int BAD_PAST_END = 3;
PPFS_HD inline bool write_range_ok(uint64_t file_size, uint64_t offset, uint64_t nbytes)
{
    return nbytes == 0 || (offset + nbytes >= offset && offset + nbytes <= file_size);
}

// files: nfiles records of sixteen dwords (the last one file_size); ranges: nfiles (offset, nbytes) pairs or
// null for every file whole.  Returns RANGE_OK, or what is wrong with file *bad, the first file that is refused.
// write: the batch is a write, whose ranges must also pass write_range_ok (BAD_PAST_END); one that passes is never
// clamped, so the slots, records and rows are the read's.
inline int build(const uint32_t* files, const uint64_t* ranges, uint64_t nfiles, uint64_t ds, Plan& p, uint64_t* bad,
    bool write = false)
{
    p = Plan {};
    p.slots.resize(nfiles);
    p.recs.resize(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint32_t* rec = files + 16u * f;
        const uint64_t offset = ranges ? ranges[2u * f] : 0u, nbytes = ranges ? ranges[2u * f + 1u] : rec[15];
        const int r = write && !write_range_ok(rec[15], offset, nbytes) ? BAD_PAST_END
                                                                        : next_slot(rec[15], ds, offset, nbytes, p.total, p.slots[f]);
        if (r != RANGE_OK) {
            if (bad)
                *bad = f;
            return r;
        }
        const Slot& s = p.slots[f];
        for (int l = 0; l < LEVELS; ++l)
            if ((l < 3 ? s.tree_n[l] : s.blocks) > 0)
                p.rows[l].push_back(Row { l < 3 ? s.tree_pos[l] : s.block_pos, (uint32_t)f, 0 });
        add_slot(p.total, s);
    }
    p.levels = levels_of(p.total);
    for (int l = 0; l < LEVELS; ++l)
        p.rows[l].push_back(Row { p.count(l), (uint32_t)nfiles, 0 });
    for (uint64_t f = 0; f < nfiles; ++f) {
        p.recs[f] = rec_of(files + 16u * f, p.slots[f], ds ? (ranges ? ranges[2u * f] : 0u) % ds : 0u, p.levels);
        level_major(p.slots[f], p.total);
    }
    return RANGE_OK;
}

// The plan of ONE file whose range is already known as blocks -- its file blocks [first, first + count), of which
// `bytes` bytes from payload byte off0 of the first are the call's (the single-file calls, which check their ranges
// themselves): what build() yields for a batch of that one file and the equivalent byte range, in a fixed record
// without a heap allocation, and the Tree of the range, which a batch's kernels rebuild per lane.
struct OneRec {
    FileRec rec;
    fileplan::Tree tree;
};
struct OnePlan {
    Slot slot;
    OneRec one;
    Row rows[LEVELS][2];
    Totals total;
    Levels levels;
    PlanView view() const
    {
        PlanView v { &one.rec, 1, {}, {}, total, levels, &one };
        for (int l = 0; l < LEVELS; ++l) {
            v.rows[l] = rows[l];
            v.nrows[l] = rows[l][0].file == 0 ? 1 : 0;
        }
        return v;
    }
};
inline void build_one(const uint32_t* inode, uint64_t first, uint64_t count, uint64_t off0, uint64_t bytes, uint64_t ds, OnePlan& p)
{
    p = OnePlan {};
    const fileplan::Tree t = fileplan::tree_of(first, count, fileplan::ipb_of(ds));
    p.slot = Slot { first, count, bytes, 0, 0, { 0, 0, 0 }, { t.nA, t.nB, t.nC } };
    add_slot(p.total, p.slot);
    p.levels = levels_of(p.total);
    p.one = OneRec { rec_of(inode, p.slot, off0, p.levels), t };
    level_major(p.slot, p.total);
    for (int l = 0; l < LEVELS; ++l) {
        const uint64_t n = l < 3 ? p.total.tree[l] : p.total.blocks;
        p.rows[l][0] = n ? Row { 0, 0, 0 } : Row { 0, 1, 0 }; // an empty level holds the sentinel alone
        p.rows[l][1] = Row { n, 1, 0 };
    }
}

// ---- the write side, host only: the plan of a batch write, and the repeat rule of its device form ----
inline int build_write(const uint32_t* files, const uint64_t* ranges, uint64_t nfiles, uint64_t ds, Plan& p, uint64_t* bad)
{
    return build(files, ranges, nfiles, ds, p, bad, true);
}

// Two ranges of the SAME inode record (64 identical bytes) whose file-block spans [first, first + blocks)
// intersect would write one block twice in one device call, where one of the writes is silently lost.  Returns
// the smallest f for which an earlier g < f has the same record and an intersecting span, or nfiles when
// there is none.  Spans that merely touch do not intersect; empty ranges take no part.  O(n log n): the
// files sorted by record (batch order within equal records), then per record the spans go into an ordered map
// in batch order -- while the spans so far are disjoint, a new one intersects some span exactly when it
// intersects its neighbour on either side.
inline uint64_t first_repeat(const Plan& p)
{
    const uint64_t n = p.recs.size();
    std::vector<uint32_t> order;
    order.reserve(n);
    for (uint64_t f = 0; f < n; ++f)
        if (p.recs[f].blocks)
            order.push_back((uint32_t)f);
    // a 64-bit hash leads the sort key, so that almost every comparison is one of two integers; equal hashes
    // fall back on the 64 bytes themselves
    std::vector<uint64_t> hash(n, 0);
    for (uint32_t f : order) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (int d = 0; d < 16; ++d)
            h = (h ^ p.recs[f].inode[d]) * 0x100000001b3ull;
        hash[f] = h;
    }
    const auto record_cmp = [&](uint32_t a, uint32_t b) {
        return hash[a] != hash[b] ? (hash[a] < hash[b] ? -1 : 1) : std::memcmp(p.recs[a].inode, p.recs[b].inode, 64);
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const int c = record_cmp(a, b);
        return c ? c < 0 : a < b;
    });
    uint64_t found = n;
    std::map<uint64_t, uint64_t> spans; // first -> end, disjoint
    for (size_t i = 0; i < order.size(); ++i) {
        const bool fresh = i == 0 || record_cmp(order[i - 1], order[i]) != 0;
        if (fresh)
            spans.clear();
        if (fresh && (i + 1 == order.size() || record_cmp(order[i], order[i + 1]) != 0))
            continue; // the only range of its record
        const uint32_t f = order[i];
        if (f >= found)
            continue; // cannot lower the answer; later files of this record are later still
        const uint64_t lo = p.recs[f].first, hi = lo + p.recs[f].blocks;
        const auto next = spans.lower_bound(lo); // the first span starting at or after lo
        bool hit = next != spans.end() && next->first < hi;
        if (!hit && next != spans.begin()) {
            auto before = next;
            --before;
            hit = before->second > lo;
        }
        if (hit)
            found = f;
        else
            spans.emplace(lo, hi);
    }
    return found;
}

} // namespace filesplan
} // namespace ppfs
