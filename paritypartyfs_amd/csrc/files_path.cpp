// files_path.cpp -- the read-only walk over a batch of files of the ppfs_ecc C ABI (include/ppfs_ecc.h):
// ppfs_ecc_files_plan, ppfs_ecc_files_blocks_* and ppfs_ecc_read_files_*.  They are file_path.cpp's calls
// applied to many inodes at once: level A of all the files is one list, level B one list, level C one list
// and the data blocks one extent stream (files_plan.hpp), so the number of launches is that of one file.
//   plan    on the host: every file's span, its places in the batch's arrays, the merged levels, per level a
//           table of (first entry, file) rows and one 128-byte record per file
//   upload  the tables go through a page-locked buffer into the call's share of the scrub scratch, on the
//           caller's stream; the buffer returns to the cache once an event behind that copy has completed
//   tree    per level A, B, C over the whole batch: expand (files_walk.hip), ONE ppfs_ecc_decode_list_*,
//           merge (statuses, counts, file flags, the caller's level-major arrays)
//   blocks  per piece of fileplan::PIECE_BLOCKS merged file blocks, cut regardless of file boundaries:
//           expand; for a read also extents, ppfs_ecc_read_extents_* into the batch's out, merge
//   write   ppfs_ecc_write_files_*: the same plan under the stricter range rule (a write stays inside the file),
//           per piece expand, extents, ppfs_ecc_write_extents_* out of the batch's in, the write merge; the
//           device form first refuses two ranges of one inode record that share a file block
// The device forms queue all of it on the caller's stream and read nothing back.  The host forms run the
// same merged plan on the CPU around the *_host list and extent calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#pragma GCC visibility push(hidden) // the plan's out-of-line inlines are no part of the library's ABI
#include "files_plan.hpp"
#pragma GCC visibility pop
#include "kernels.hpp"
#include "list_call.hpp"

using namespace ppfs;
using namespace ppfs::fileplan;
using filesplan::FileRec;
using filesplan::Plan;
using filesplan::Row;

static_assert(sizeof(ppfs_ecc_file_range) == 16, "a range is two 64-bit words");
static_assert(sizeof(ppfs_ecc_files_slot) == sizeof(filesplan::Slot) && sizeof(ppfs_ecc_files_slot) == 88, "slot layout");
static_assert(sizeof(ppfs_ecc_files_totals) == sizeof(filesplan::Totals) && sizeof(ppfs_ecc_files_totals) == 48, "totals layout");

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t blocks_seen(size_t image_blocks) { return std::min<size_t>(image_blocks, NO_BLOCK); } // NO_BLOCK names no block

// The checks of a batch that need no GPU, and its plan
int batch_args(const ppfs_ecc_ctx* c, const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles, const char* who,
    Plan& plan)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null context").c_str());
    if (nfiles && !files)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null file records").c_str());
    if (nfiles >= 0xFFFFFFFFull)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": a batch holds fewer than 2^32 - 1 files").c_str());
    uint64_t bad = 0;
    const int r = filesplan::build((const uint32_t*)files, (const uint64_t*)ranges, nfiles, c->data, plan, &bad);
    if (r == filesplan::BAD_OFFSET)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": file " + std::to_string(bad) + ": offset at or past the file's end").c_str());
    if (r != filesplan::RANGE_OK)
        return fail(PPFS_ECC_EINVAL,
            (std::string(who) + ": file " + std::to_string(bad) + ": the range's blocks pass the tree's capacity").c_str());
    return 0;
}
// ... and of a walk's or a read's buffers
int walk_args(const ppfs_ecc_ctx* c, const void* image, const Plan& plan, const void* index, const void* tree_index, const void* flags,
    const void* counts, const char* who)
{
    if ((((uintptr_t)index | (uintptr_t)tree_index | (uintptr_t)flags) & 3u) || ((uintptr_t)counts & 7u))
        return fail(PPFS_ECC_EINVAL,
            (std::string(who) + ": index and flags arrays are 4-byte, the counts record 8-byte aligned").c_str());
    if (plan.total.blocks && !image)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null image").c_str());
    return 0;
}
int read_args(const ppfs_ecc_ctx* c, const void* image, const Plan& plan, const void* out, uint64_t out_bytes, const void* flags,
    const void* counts, const char* who)
{
    if (c->data > 0xFFFFu)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": payloads past 65,535 bytes do not fit an extent").c_str());
    const int r = walk_args(c, image, plan, nullptr, nullptr, flags, counts, who);
    if (r)
        return r;
    if (plan.total.blocks && (!out || out_bytes < plan.total.bytes))
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": the out buffer is null or shorter than the bytes to deliver").c_str());
    return 0;
}

// The checks of a batch WRITE that need no GPU, and its plan: ppfs_ecc_files_plan's slots under the stricter range
// rule (filesplan::build_write); distinct: also refuse two ranges of one inode record that share a file block
int write_args(const ppfs_ecc_ctx* c, const void* image, const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles,
    const void* in, uint64_t in_bytes, const void* flags, const void* written, const void* counts, bool distinct, const char* who,
    Plan& plan)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null context").c_str());
    if (nfiles && !files)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null file records").c_str());
    if (nfiles >= 0xFFFFFFFFull)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": a batch holds fewer than 2^32 - 1 files").c_str());
    uint64_t bad = 0;
    const int b = filesplan::build_write((const uint32_t*)files, (const uint64_t*)ranges, nfiles, c->data, plan, &bad);
    if (b != filesplan::RANGE_OK)
        return fail(PPFS_ECC_EINVAL,
            (std::string(who) + ": file " + std::to_string(bad)
                + (b == filesplan::BAD_CAPACITY ? ": the range's blocks pass the tree's capacity"
                                                : ": the range runs past the file's end (a write does not grow the file)"))
                .c_str());
    if ((uintptr_t)written & 7u)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": the written array is 8-byte aligned").c_str());
    if (c->data > 0xFFFFu)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": payloads past 65,535 bytes do not fit an extent").c_str());
    const int r = walk_args(c, image, plan, nullptr, nullptr, flags, counts, who);
    if (r)
        return r;
    if (plan.total.blocks && (!in || in_bytes < plan.total.bytes))
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": the in buffer is null or shorter than the bytes to write").c_str());
    if (distinct) {
        const uint64_t f = filesplan::first_repeat(plan);
        if (f < nfiles)
            return fail(PPFS_ECC_EINVAL,
                (std::string(who) + ": file " + std::to_string(f)
                    + ": its range shares a file block with an earlier range of the same inode (device writes need distinct blocks)")
                    .c_str());
    }
    return 0;
}

// where a level starts in the caller's level-major tree arrays
uint64_t entry_base(const Plan& p, int level) { return level == LEVEL_A ? 0u : level == LEVEL_B ? p.total.tree[0] : p.total.tree[0] + p.total.tree[1]; }

// ------------------------------------------------------------------------------------------------------
// Device side
// ------------------------------------------------------------------------------------------------------
// A call's share of the context's scrub scratch: the tables (the records, then the four row tables), the
// merged tree as in file_path.cpp (pointer, decode status, inherited status, payload per slot), a piece of
// merged file blocks (pointer, path status, extent, read status).
struct Scratch {
    uint8_t* tables;
    uint32_t* tidx;
    uint8_t *tst, *tinh, *tpay;
    uint32_t* idx;
    uint8_t* path;
    ppfs_ecc_extent* ext;
    uint8_t* rst;
};
struct TableLayout {
    size_t recs, rows[filesplan::LEVELS], bytes;
};
TableLayout table_layout(const Plan& p)
{
    TableLayout t {};
    t.recs = 0;
    size_t at = round_up(p.recs.size() * sizeof(FileRec), 256);
    for (int l = 0; l < filesplan::LEVELS; ++l) {
        t.rows[l] = at;
        at = round_up(at + p.rows[l].size() * sizeof(Row), 256);
    }
    t.bytes = at;
    return t;
}
size_t scratch_layout(const Plan& p, size_t table_bytes, size_t ds, size_t piece, bool read, uint8_t* base, Scratch* s)
{
    const size_t slots = p.levels.slots;
    const size_t o_tidx = round_up(table_bytes, 256), o_tst = round_up(o_tidx + slots * 4, 256), o_tinh = round_up(o_tst + slots, 256),
                 o_tpay = round_up(o_tinh + slots, 256), o_idx = round_up(o_tpay + slots * ds + 16, 256),
                 o_path = round_up(o_idx + piece * 4, 256), o_ext = round_up(o_path + piece, 256),
                 o_rst = round_up(o_ext + (read ? piece * 16 : 0), 256),
                 bytes = round_up(o_rst + (read ? piece : 0), 256); // the codecs store statuses in whole 16-byte windows
    if (s)
        *s = Scratch { base, (uint32_t*)(base + o_tidx), base + o_tst, base + o_tinh, base + o_tpay, (uint32_t*)(base + o_idx),
            base + o_path, (ppfs_ecc_extent*)(base + o_ext), base + o_rst };
    return bytes;
}

// page-locked buffers of earlier batch calls whose copy has completed go back to the cache
void reap_stages(ppfs_ecc_ctx* c)
{
    auto& v = c->files_stage;
    for (size_t i = 0; i < v.size();) {
        const hipError_t e = hipEventQuery(v[i].done);
        if (e == hipErrorNotReady) {
            ++i;
            continue;
        }
        if (e != hipSuccess) { // a failed query says nothing about the copy: wait for it
            (void)hipGetLastError();
            (void)hipEventSynchronize(v[i].done);
        }
        (void)hipEventDestroy(v[i].done);
        pin_free(v[i].buf, v[i].bytes, kPinStage);
        v[i] = v.back();
        v.pop_back();
    }
}

struct DeviceBatch {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t blocks;
    const Plan& plan;
    size_t ds;
    int wb;
    void* stream;
    Scratch x {};
    TableLayout tl {};
    hipStream_t s() const { return (hipStream_t)stream; }
    uint64_t nfiles() const { return plan.recs.size(); }
    const void* rows(int level) const { return x.tables + tl.rows[level]; }
    uint64_t nrows(int level) const { return plan.rows[level].size() - 1; }

    // the scratch (after a wait for its previous user), then the tables into it through a page-locked
    // buffer that outlives the copy
    int setup(size_t piece, bool read)
    {
        reap_stages(c);
        tl = table_layout(plan);
        uint8_t* scratch = nullptr;
        int r = scrub_scratch(c, scratch_layout(plan, tl.bytes, ds, piece, read, nullptr, nullptr), s(), &scratch);
        if (r)
            return r;
        scratch_layout(plan, tl.bytes, ds, piece, read, scratch, &x);
        size_t cap = 4096; // few distinct sizes, so that the cache of page-locked buffers hits
        while (cap < tl.bytes)
            cap *= 2;
        uint8_t* pin = nullptr;
        if (pin_alloc((void**)&pin, cap, kPinStage) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PPFS_ECC_ENOMEM, "files: page-locked staging of the tables");
        }
        std::memcpy(pin + tl.recs, plan.recs.data(), plan.recs.size() * sizeof(FileRec));
        for (int l = 0; l < filesplan::LEVELS; ++l)
            std::memcpy(pin + tl.rows[l], plan.rows[l].data(), plan.rows[l].size() * sizeof(Row));
        hipError_t e = dma_async(x.tables, pin, tl.bytes, hipMemcpyHostToDevice, s());
        hipEvent_t done = nullptr;
        if (e == hipSuccess && (e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) == hipSuccess
            && (e = hipEventRecord(done, s())) == hipSuccess) {
            c->files_stage.push_back(ppfs_ecc_ctx::FilesStage { pin, cap, done });
            return 0;
        }
        // nothing to tell the copy's end by: drain the stream, then the buffer is free
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s());
        if (done)
            (void)hipEventDestroy(done);
        pin_free(pin, cap, kPinStage);
        return fail(PPFS_ECC_EHIP, "files: table upload", e);
    }
    int expand(int level, uint64_t e0, uint64_t n, uint32_t* pointer, uint8_t* inherited) const
    {
        return check_hip(ppfs_files_expand_launch(x.tables + tl.recs, nfiles(), rows(level), nrows(level), level, e0, n, ds, x.tpay,
                             x.tst, x.tinh, plan.levels.slots, pointer, inherited, s()),
            "files expand");
    }
    int merge(int level, const uint8_t* path, const uint8_t* read, uint64_t e0, uint64_t n, uint8_t* status_out,
        const uint32_t* pointer_in, uint32_t* pointer_out, uint8_t* out, uint32_t* flags, unsigned long long* counts) const
    {
        const bool tree = level != LEVEL_DATA;
        return check_hip(ppfs_files_merge_launch(x.tables + tl.recs, nfiles(), rows(level), nrows(level), path, read, e0, n, status_out,
                             pointer_in, pointer_out, out, plan.total.bytes, ds, flags, tree ? filesplan::FLAG_TREE_SHIFT : 0u, counts,
                             tree ? SLOT_INDEX : SLOT_FILE, s()),
            "files merge");
    }
    // levels A, B, C of the whole batch: each one list decode; the caller's arrays level-major (either may be null)
    int levels(uint32_t* tree_index, uint8_t* tree_status, uint32_t* flags, unsigned long long* counts) const
    {
        int r = 0;
        for (int level = LEVEL_A; level <= LEVEL_C && !r; ++level) {
            const uint64_t n = plan.total.tree[level], at = plan.levels.base[level], to = entry_base(plan, level);
            if (n == 0)
                continue;
            (void)((r = expand(level, 0, n, x.tidx + at, x.tinh + at))
                || (r = ppfs_ecc_decode_list_device(c, image, blocks, x.tidx + at, n, x.tpay + at * ds, x.tst + at, wb, nullptr, stream))
                || (r = merge(level, x.tinh + at, x.tst + at, 0, n, tree_status ? tree_status + to : nullptr, x.tidx + at,
                        tree_index ? tree_index + to : nullptr, nullptr, flags, counts)));
        }
        return r;
    }
};

// what both device forms do before the walk: refuse a capture, clear the counts and the flags
int device_begin(hipStream_t s, size_t nfiles, uint32_t* d_flags, ppfs_ecc_file_counts* d_counts)
{
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "file calls cannot be captured into a graph (shared scratch and staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "files counts clear");
    if (d_flags && nfiles)
        HIP_TRY(hipMemsetAsync(d_flags, 0, nfiles * sizeof(uint32_t), s), "files flags clear");
    return 0;
}

void slots_out(const Plan& plan, ppfs_ecc_files_slot* slots, ppfs_ecc_files_totals* totals)
{
    if (slots && !plan.slots.empty())
        std::memcpy(slots, plan.slots.data(), plan.slots.size() * sizeof(filesplan::Slot));
    if (totals)
        std::memcpy(totals, &plan.total, sizeof(*totals));
}

} // namespace

extern "C" int ppfs_ecc_files_plan(const ppfs_ecc_ctx* c, const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles,
    ppfs_ecc_files_slot* slots, ppfs_ecc_files_totals* totals)
{
    Plan plan;
    const int r = batch_args(c, files, ranges, nfiles, "files plan", plan);
    if (r)
        return r;
    slots_out(plan, slots, totals);
    return 0;
}

extern "C" int ppfs_ecc_files_blocks_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint32_t* d_index, uint8_t* d_path_status, uint32_t* d_tree_index,
    uint8_t* d_tree_status, uint32_t* d_file_flags, ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Plan plan;
    int r = batch_args(c, files, ranges, nfiles, "files blocks", plan);
    if (r || (r = walk_args(c, d_image, plan, d_index, d_tree_index, d_file_flags, d_counts, "files blocks")))
        return r;
    hipStream_t s = (hipStream_t)stream;
    if ((r = device_begin(s, nfiles, d_file_flags, d_counts)))
        return r;
    const uint64_t nblocks = plan.total.blocks;
    if (nblocks == 0)
        return 0;
    unsigned long long* counts = (unsigned long long*)d_counts;
    DeviceBatch w { c, d_image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(nblocks, PIECE_BLOCKS);
    if ((r = w.setup(piece, false)))
        return r;
    r = w.levels(d_tree_index, d_tree_status, d_file_flags, counts);
    if (d_index || d_path_status || counts || d_file_flags) {
        for (uint64_t off = 0; off < nblocks && !r; off += piece) {
            const uint64_t nb = std::min<uint64_t>(piece, nblocks - off);
            uint8_t* path = d_path_status ? d_path_status + off : w.x.path;
            (void)((r = w.expand(LEVEL_DATA, off, nb, d_index ? d_index + off : nullptr, path))
                || (r = w.merge(LEVEL_DATA, path, nullptr, off, nb, nullptr, nullptr, nullptr, nullptr, d_file_flags, counts)));
        }
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, nblocks, stream, "files blocks (async)");
}

extern "C" int ppfs_ecc_read_files_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, uint32_t* d_file_flags,
    ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Plan plan;
    int r = batch_args(c, files, ranges, nfiles, "read files", plan);
    if (r || (r = read_args(c, d_image, plan, d_out, out_bytes, d_file_flags, d_counts, "read files")))
        return r;
    hipStream_t s = (hipStream_t)stream;
    if ((r = device_begin(s, nfiles, d_file_flags, d_counts)))
        return r;
    const uint64_t nblocks = plan.total.blocks;
    if (nblocks == 0)
        return 0;
    unsigned long long* counts = (unsigned long long*)d_counts;
    DeviceBatch w { c, d_image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(nblocks, PIECE_BLOCKS);
    if ((r = w.setup(piece, true)))
        return r;
    r = w.levels(nullptr, nullptr, d_file_flags, counts);
    for (uint64_t off = 0; off < nblocks && !r; off += piece) {
        const uint64_t nb = std::min<uint64_t>(piece, nblocks - off);
        (void)((r = w.expand(LEVEL_DATA, off, nb, w.x.idx, w.x.path))
            || (r = check_hip(ppfs_files_extents_launch(w.x.tables + w.tl.recs, w.nfiles(), w.rows(LEVEL_DATA), w.nrows(LEVEL_DATA),
                                  w.x.idx, w.x.path, off, nb, w.ds, w.x.ext, s),
                    "files extents"))
            || (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, w.x.ext, nb, d_out, plan.total.bytes, w.x.rst, w.wb, stream))
            || (r = w.merge(LEVEL_DATA, w.x.path, w.x.rst, off, nb, d_status ? d_status + off : nullptr, nullptr, nullptr, d_out,
                    d_file_flags, counts)));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, nblocks, stream, "read files (async)");
}

// FileIO::writeFile over an existing range (file_io.cpp:46-104) for every file of a batch: the read's walk and
// extents with pos pointing into `in`, ppfs_ecc_write_extents_device per piece, then the write merge
extern "C" int ppfs_ecc_write_files_device(ppfs_ecc_ctx* c, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* d_status,
    uint32_t* d_file_flags, uint64_t* d_written, ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Plan plan;
    int r = write_args(c, d_image, files, ranges, nfiles, d_in, in_bytes, d_file_flags, d_written, d_counts, true, "write files", plan);
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if ((r = device_begin(s, nfiles, d_file_flags, d_counts)))
        return r;
    const uint64_t nblocks = plan.total.blocks;
    unsigned long long *counts = (unsigned long long*)d_counts, *written = (unsigned long long*)d_written;
    if (nblocks == 0) { // every range is empty: nothing is written, of nothing
        if (written && nfiles)
            HIP_TRY(hipMemsetAsync(written, 0, nfiles * sizeof(uint64_t), s), "files written clear");
        return 0;
    }
    DeviceBatch w { c, d_image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(nblocks, PIECE_BLOCKS);
    if ((r = w.setup(piece, true)))
        return r;
    (void)((r = check_hip(ppfs_files_written_init_launch(w.x.tables + w.tl.recs, w.nfiles(), written, s), "files written init"))
        || (r = w.levels(nullptr, nullptr, d_file_flags, counts)));
    for (uint64_t off = 0; off < nblocks && !r; off += piece) {
        const uint64_t nb = std::min<uint64_t>(piece, nblocks - off);
        (void)((r = w.expand(LEVEL_DATA, off, nb, w.x.idx, w.x.path))
            || (r = check_hip(ppfs_files_extents_launch(w.x.tables + w.tl.recs, w.nfiles(), w.rows(LEVEL_DATA), w.nrows(LEVEL_DATA),
                                  w.x.idx, w.x.path, off, nb, w.ds, w.x.ext, s),
                    "files extents"))
            || (r = ppfs_ecc_write_extents_device(c, d_in, plan.total.bytes, d_image, image_blocks, w.x.ext, nb, w.x.rst, stream))
            || (r = check_hip(ppfs_files_write_merge_launch(w.x.tables + w.tl.recs, w.nfiles(), w.rows(LEVEL_DATA),
                                  w.nrows(LEVEL_DATA), w.x.path, w.x.rst, off, nb, d_status ? d_status + off : nullptr, w.ds,
                                  d_file_flags, written, counts, s),
                    "files write merge")));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, nblocks, stream, "write files (async)");
}

// ------------------------------------------------------------------------------------------------------
// Host side: the same merged plan on the CPU
// ------------------------------------------------------------------------------------------------------
namespace {

struct HostMem {
    const uint8_t *payload, *st, *inh;
    uint32_t status(uint64_t p) const { return st[p]; }
    uint32_t inherited(uint64_t p) const { return inh[p]; }
    uint32_t payload_byte(uint64_t at) const { return payload[at]; }
};

struct HostBatch {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t blocks;
    const Plan& plan;
    size_t ds;
    int wb;
    uint32_t* flags;
    ppfs_ecc_file_counts* counts;
    std::vector<uint32_t> tidx;
    std::vector<uint8_t> tst, tinh, tpay;

    HostMem mem() const { return HostMem { tpay.data(), tst.data(), tinh.data() }; }
    void note(uint32_t file, uint32_t st, bool tree)
    {
        const int slot = count_slot(st);
        if (counts && slot >= 0)
            ++(&counts->ok)[(tree ? SLOT_INDEX : SLOT_FILE) + slot];
        if (flags)
            flags[file] |= filesplan::flag_of(st) << (tree ? filesplan::FLAG_TREE_SHIFT : 0u);
    }
    // fn(file, k, merged entry) for every entry of a level, in merged order
    template <class Fn>
    void each(int level, Fn fn) const
    {
        const std::vector<Row>& rows = plan.rows[level];
        for (size_t r = 0; r + 1 < rows.size(); ++r)
            for (uint64_t e = rows[r].first; e < rows[r + 1].first; ++e)
                fn(rows[r].file, e - rows[r].first, e);
    }
    int levels(uint32_t* tree_index, uint8_t* tree_status)
    {
        const size_t slots = plan.levels.slots;
        tidx.assign(slots, NO_BLOCK);
        tst.assign(slots, 0);
        tinh.assign(slots, 0);
        tpay.assign(slots * ds, 0);
        for (int level = LEVEL_A; level <= LEVEL_C; ++level) {
            const uint64_t n = plan.total.tree[level], at = plan.levels.base[level], to = entry_base(plan, level);
            if (n == 0)
                continue;
            const HostMem m = mem();
            each(level, [&](uint32_t f, uint64_t k, uint64_t e) {
                const Expanded x = filesplan::expand_entry(plan.recs[f], level, k, ds, m);
                tidx[at + e] = x.pointer;
                tinh[at + e] = x.inherited;
            });
            const int r = ppfs_ecc_decode_list_host(c, image, blocks, tidx.data() + at, n, tpay.data() + at * ds, tst.data() + at, wb,
                nullptr);
            if (r)
                return r;
            each(level, [&](uint32_t f, uint64_t, uint64_t e) {
                const uint8_t st = tinh[at + e] ? tinh[at + e] : tst[at + e];
                if (tree_index)
                    tree_index[to + e] = tidx[at + e];
                if (tree_status)
                    tree_status[to + e] = st;
                note(f, st, true);
            });
        }
        return 0;
    }
};

void host_begin(size_t nfiles, uint32_t* flags, ppfs_ecc_file_counts* counts)
{
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (flags && nfiles)
        std::memset(flags, 0, nfiles * sizeof(uint32_t));
}

} // namespace

extern "C" int ppfs_ecc_files_blocks_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint32_t* index, uint8_t* path_status, uint32_t* tree_index,
    uint8_t* tree_status, uint32_t* file_flags, ppfs_ecc_file_counts* counts, int write_back)
{
    Plan plan;
    int r = batch_args(c, files, ranges, nfiles, "files blocks (host)", plan);
    if (r || (r = walk_args(c, image, plan, index, tree_index, file_flags, counts, "files blocks (host)")))
        return r;
    host_begin(nfiles, file_flags, counts);
    if (plan.total.blocks == 0)
        return 0;
    HostBatch w { c, image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, file_flags, counts, {}, {}, {}, {} };
    if ((r = w.levels(tree_index, tree_status)))
        return r;
    const HostMem m = w.mem();
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t k, uint64_t e) {
        const Expanded x = filesplan::expand_entry(plan.recs[f], LEVEL_DATA, k, w.ds, m);
        if (index)
            index[e] = x.pointer;
        if (path_status)
            path_status[e] = x.inherited;
        w.note(f, x.inherited, false);
    });
    return 0;
}

extern "C" int ppfs_ecc_read_files_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* out, size_t out_bytes, uint8_t* status, uint32_t* file_flags,
    ppfs_ecc_file_counts* counts, int write_back)
{
    Plan plan;
    int r = batch_args(c, files, ranges, nfiles, "read files (host)", plan);
    if (r || (r = read_args(c, image, plan, out, out_bytes, file_flags, counts, "read files (host)")))
        return r;
    host_begin(nfiles, file_flags, counts);
    const uint64_t nblocks = plan.total.blocks;
    if (nblocks == 0)
        return 0;
    HostBatch w { c, image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, file_flags, counts, {}, {}, {}, {} };
    if ((r = w.levels(nullptr, nullptr)))
        return r;
    const HostMem m = w.mem();
    std::vector<ppfs_ecc_extent> ext(nblocks);
    std::vector<uint8_t> path(nblocks), rst(nblocks);
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t k, uint64_t e) {
        const FileRec& rec = plan.recs[f];
        const Expanded x = filesplan::expand_entry(rec, LEVEL_DATA, k, w.ds, m);
        const Extent at = extent_of(k, rec.off0, rec.bytes, w.ds);
        path[e] = x.inherited;
        ext[e] = ppfs_ecc_extent { rec.out_pos + at.pos, x.inherited ? NO_BLOCK : x.pointer, (uint16_t)at.offset, (uint16_t)at.length };
    });
    if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), nblocks, out, plan.total.bytes, rst.data(), w.wb)))
        return r;
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t, uint64_t e) {
        const uint8_t st = path[e] ? path[e] : rst[e];
        if (status)
            status[e] = st;
        if (path[e] == STATUS_FAILED)
            std::memset(out + ext[e].pos, 0, ext[e].length);
        w.note(f, st, false);
    });
    return 0;
}

// Repeats are not refused here: ppfs_ecc_write_extents_host cuts its list where a block repeats, so the ranges apply
// in batch order
extern "C" int ppfs_ecc_write_files_host(ppfs_ecc_ctx* c, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_file* files, const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* status, uint32_t* file_flags,
    uint64_t* written, ppfs_ecc_file_counts* counts, int write_back)
{
    Plan plan;
    int r = write_args(c, image, files, ranges, nfiles, in, in_bytes, file_flags, written, counts, false, "write files (host)", plan);
    if (r)
        return r;
    host_begin(nfiles, file_flags, counts);
    if (written)
        for (size_t f = 0; f < nfiles; ++f)
            written[f] = plan.recs[f].bytes;
    const uint64_t nblocks = plan.total.blocks;
    if (nblocks == 0)
        return 0;
    HostBatch w { c, image, blocks_seen(image_blocks), plan, c->data, write_back ? 1 : 0, file_flags, counts, {}, {}, {}, {} };
    if ((r = w.levels(nullptr, nullptr)))
        return r;
    const HostMem m = w.mem();
    std::vector<ppfs_ecc_extent> ext(nblocks);
    std::vector<uint8_t> path(nblocks), wst(nblocks);
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t k, uint64_t e) {
        const FileRec& rec = plan.recs[f];
        const Expanded x = filesplan::expand_entry(rec, LEVEL_DATA, k, w.ds, m);
        const Extent at = extent_of(k, rec.off0, rec.bytes, w.ds);
        path[e] = x.inherited;
        ext[e] = ppfs_ecc_extent { rec.out_pos + at.pos, x.inherited ? NO_BLOCK : x.pointer, (uint16_t)at.offset, (uint16_t)at.length };
    });
    if ((r = ppfs_ecc_write_extents_host(c, in, plan.total.bytes, image, image_blocks, ext.data(), nblocks, wst.data())))
        return r;
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t, uint64_t e) {
        const uint8_t st = path[e] ? path[e] : wst[e];
        if (status)
            status[e] = st;
        if (written && (st == STATUS_FAILED || st == STATUS_OUT))
            written[f] = std::min<uint64_t>(written[f], ext[e].pos - plan.recs[f].out_pos);
        w.note(f, st, false);
    });
    return 0;
}
