// lookup_path.cpp -- the directory lookups of the ppfs_ecc C ABI (include/ppfs_ecc.h): ppfs_ecc_lookup_plan and
// ppfs_ecc_lookup_*, DirectoryManager::getInodeByName (lib/directory_manager/src/directory_manager.cpp:135-163) and
// the search of removeEntry (:67-90) over a batch of (directory, key).
//
// The reference's loop reads a directory 256 entries at a time and compares as it goes.  Here every directory of the
// call is read once and whole by the file batch (ppfs_ecc_read_files_* over the ranges (0, 128 n_d)) into the
// caller's entries buffer, with one final status per file block, and the queries are answered from those two arrays:
//   match    the first matching entry of every query (dir_walk.hip; on the host a plain loop)
//   finish   the loop's failure rule over the block statuses, the hit records, the tally
// The rule is lookup_plan.hpp's, for both forms.  The device form queues all of it on the caller's stream and reads
// nothing back; the per-directory table and the query records travel like the file batch's tables (stage_upload,
// files_path.cpp) into the context's scrub scratch, so no call allocates or frees on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "file_call.hpp"
#include "kernels.hpp"
#include "list_call.hpp"
#pragma GCC visibility push(hidden) // the plan's records and their containers are no part of the library's ABI
#include "lookup_plan.hpp"
#pragma GCC visibility pop

using namespace ppfs;
using namespace ppfs::lookupplan;

static_assert(sizeof(ppfs_ecc_lookup_query) == sizeof(Query) && sizeof(ppfs_ecc_lookup_hit) == sizeof(Hit), "record layouts");
static_assert(sizeof(ppfs_ecc_lookup_counts) == 64, "counts layout");
static_assert(PPFS_ECC_NOT_FOUND == ST_NOT_FOUND, "the header's status is the plan's");

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What a call knows before anything touches the GPU: the ranges (0, 128 n_d), the file batch's slots over them and
// the per-directory table
struct Dirs {
    std::vector<ppfs_ecc_file_range> ranges;
    std::vector<ppfs_ecc_files_slot> slots;
    ppfs_ecc_files_totals total {};
    std::vector<DirRec> recs;
    uint64_t max_entries = 0;
};
int plan_dirs(const ppfs_ecc_ctx* c, const ppfs_ecc_file* dirs, size_t ndirs, const char* who, Dirs& d)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null context").c_str());
    if (ndirs && !dirs)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null directory records").c_str());
    d.ranges.resize(ndirs);
    d.slots.resize(ndirs);
    d.recs.resize(ndirs);
    for (size_t i = 0; i < ndirs; ++i) {
        const uint64_t n = entries_of(((const uint32_t*)(dirs + i))[15]);
        d.ranges[i] = ppfs_ecc_file_range { 0, (uint64_t)ENTRY_BYTES * n };
        d.recs[i].n = n;
        d.max_entries = std::max(d.max_entries, n);
    }
    const int r = ppfs_ecc_files_plan(c, dirs, d.ranges.data(), ndirs, d.slots.data(), &d.total);
    if (r)
        return r;
    for (size_t i = 0; i < ndirs; ++i) {
        d.recs[i].out_pos = d.slots[i].out_pos;
        d.recs[i].block_pos = d.slots[i].block_pos;
        d.recs[i].blocks = d.slots[i].blocks;
    }
    return 0;
}

// the checks of a lookup that need no GPU; device: the working buffers are required
int lookup_args(const ppfs_ecc_ctx* c, const void* image, const ppfs_ecc_file* dirs, size_t ndirs, const ppfs_ecc_lookup_query* queries,
    const void* names, size_t nq, int mode, const void* entries, size_t entries_bytes, const void* block_status, const void* dir_flags,
    const void* hits, const void* counts, const void* file_counts, bool device, const char* who, Dirs& d)
{
    auto bad = [&](const std::string& what) { return fail(PPFS_ECC_EINVAL, (std::string(who) + ": " + what).c_str()); };
    if (!c)
        return bad("null context");
    if (mode != MODE_NAME && mode != MODE_INODE)
        return bad("mode is 0 (name) or 1 (inode number)");
    if ((((uintptr_t)hits | (uintptr_t)dir_flags) & 3u) || (((uintptr_t)counts | (uintptr_t)file_counts) & 7u))
        return bad("hits and flags are 4-byte, the counts records 8-byte aligned");
    if (nq == 0)
        return 0;
    if (!image || !dirs || !queries || !hits)
        return bad("null image, directory records, queries or hits");
    if (mode == MODE_NAME && !names)
        return bad("null names in name mode");
    if (nq >= 0xFFFFFFFFull)
        return bad("a call holds fewer than 2^32 - 1 queries");
    for (size_t q = 0; q < nq; ++q)
        if (queries[q].dir >= ndirs)
            return bad("query " + std::to_string(q) + ": its directory is at or past ndirs");
    const int r = plan_dirs(c, dirs, ndirs, who, d);
    if (r)
        return r;
    if (device && d.total.blocks && (!entries || !block_status))
        return bad("the entries buffer and the block status array are the call's working memory: both are required");
    if (entries && entries_bytes < d.total.bytes)
        return bad("the entries buffer is shorter than the directories' entries");
    return 0;
}

} // namespace

extern "C" int ppfs_ecc_lookup_plan(const ppfs_ecc_ctx* c, const ppfs_ecc_file* dirs, size_t ndirs, ppfs_ecc_files_slot* slots,
    ppfs_ecc_files_totals* totals)
{
    Dirs d;
    const int r = plan_dirs(c, dirs, ndirs, "lookup plan", d);
    if (r)
        return r;
    if (slots && ndirs)
        std::memcpy(slots, d.slots.data(), ndirs * sizeof(*slots));
    if (totals)
        *totals = d.total;
    return 0;
}

extern "C" int ppfs_ecc_lookup_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* dirs, size_t ndirs,
    const ppfs_ecc_lookup_query* queries, const uint8_t* d_names, size_t nq, int mode, uint8_t* d_entries, size_t entries_bytes,
    uint8_t* d_block_status, uint32_t* d_dir_flags, ppfs_ecc_lookup_hit* d_hits, ppfs_ecc_lookup_counts* d_counts,
    ppfs_ecc_file_counts* d_file_counts, int write_back, void* stream)
{
    Dirs d;
    int r = lookup_args(c, d_image, dirs, ndirs, queries, d_names, nq, mode, d_entries, entries_bytes, d_block_status, d_dir_flags, d_hits,
        d_counts, d_file_counts, true, "lookup", d);
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "lookup calls cannot be captured into a graph (shared scratch and staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "lookup counts clear");
    if (nq == 0)
        return 0;
    // every directory whole: entries and final block statuses as the file batch leaves them
    if ((r = ppfs_ecc_read_files_device(c, d_image, image_blocks, dirs, d.ranges.data(), ndirs, d_entries, entries_bytes, d_block_status,
             d_dir_flags, d_file_counts, write_back, stream)))
        return r;
    (void)call_ordered(c, nq, stream);
    const size_t o_queries = round_up(ndirs * sizeof(DirRec), 256), bytes = round_up(o_queries + nq * sizeof(Query), 256);
    uint8_t* base = nullptr;
    if ((r = scrub_scratch(c, bytes, s, &base)))
        return r;
    (void)((r = stage_upload(c, base, bytes, s, "lookup",
                [&](uint8_t* pin) {
                    std::memcpy(pin, d.recs.data(), ndirs * sizeof(DirRec));
                    std::memcpy(pin + o_queries, queries, nq * sizeof(Query));
                }))
        || (r = check_hip(hipMemsetAsync(d_hits, 0xFF, nq * sizeof(*d_hits), s), "lookup hits init"))
        || (r = check_hip(ppfs_lookup_match_launch(base, ndirs, base + o_queries, d_names, nq, mode, d_entries, d.total.bytes,
                              d.max_entries, d_hits, s),
                "lookup match"))
        || (r = check_hip(ppfs_lookup_finish_launch(base, ndirs, base + o_queries, nq, d_entries, d.total.bytes, d_block_status,
                              d.total.blocks, c->data, d_hits, (unsigned long long*)d_counts, s),
                "lookup finish")));
    scrub_scratch_used(c, s);
    return call_queued(c, r, nq, stream, "lookup (async)");
}

// The same rule on the CPU around one ppfs_ecc_read_files_host
extern "C" int ppfs_ecc_lookup_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* dirs, size_t ndirs,
    const ppfs_ecc_lookup_query* queries, const uint8_t* names, size_t nq, int mode, uint8_t* entries, size_t entries_bytes,
    uint8_t* block_status, uint32_t* dir_flags, ppfs_ecc_lookup_hit* hits, ppfs_ecc_lookup_counts* counts,
    ppfs_ecc_file_counts* file_counts, int write_back)
{
    Dirs d;
    int r = lookup_args(c, image, dirs, ndirs, queries, names, nq, mode, entries, entries_bytes, block_status, dir_flags, hits, counts,
        file_counts, false, "lookup (host)", d);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_lookup_counts {};
    if (nq == 0)
        return 0;
    std::vector<uint8_t> own_entries, own_status;
    if (!entries) {
        own_entries.resize(d.total.bytes + 1);
        entries = own_entries.data();
        entries_bytes = d.total.bytes;
    }
    if (!block_status) {
        own_status.resize(d.total.blocks + 1);
        block_status = own_status.data();
    }
    if ((r = ppfs_ecc_read_files_host(c, image, image_blocks, dirs, d.ranges.data(), ndirs, entries, entries_bytes, block_status, dir_flags,
             file_counts, write_back)))
        return r;
    const uint64_t ds = c->data;
    auto le32 = [](const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; };
    // per directory its lowest failing file block, found once for all its queries
    std::vector<uint64_t> lowest(ndirs, NO_FAILURE);
    std::vector<uint8_t> lowest_status(ndirs, 0);
    for (size_t i = 0; i < ndirs; ++i)
        for (uint64_t j = 0; j < d.recs[i].blocks && lowest[i] == NO_FAILURE; ++j)
            if (fails(block_status[d.recs[i].block_pos + j])) {
                lowest[i] = j;
                lowest_status[i] = block_status[d.recs[i].block_pos + j];
            }
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t di = queries[q].dir;
        const DirRec& dir = d.recs[di];
        const uint8_t* base = entries + dir.out_pos;
        const uint8_t* name = mode == MODE_NAME ? names + (size_t)QUERY_BYTES * q : nullptr;
        auto query_word = [&](uint32_t w) { return le32(name + 4u * w); };
        const uint32_t L = name ? query_length(query_word) : 0u;
        const uint32_t m = first_match(dir.n, [&](uint64_t e) {
            const uint8_t* p = base + (uint64_t)ENTRY_BYTES * e;
            return mode == MODE_INODE ? inode_match(le32(p), queries[q].key)
                                      : name_match([&](uint32_t w) { return le32(p + 4u + 4u * w); }, query_word, L);
        });
        const uint32_t failure = dir.n ? failure_within(last_block(dir.n, m, ds), lowest[di], lowest_status[di]) : 0u;
        const Hit h = answer(dir.n, m, failure, m != NONE ? le32(base + (uint64_t)ENTRY_BYTES * m) : NONE);
        std::memcpy(hits + q, &h, sizeof(h));
        const int slot = count_slot(h.status);
        if (counts && slot >= 0)
            ++(&counts->found)[slot];
    }
    return 0;
}
