// files_path.cpp -- the file walk of the ppfs_ecc C ABI (include/ppfs_ecc.h), and its batch entry points:
// ppfs_ecc_files_plan, ppfs_ecc_files_blocks_*, ppfs_ecc_read_files_* and ppfs_ecc_write_files_*.  The single-file
// entry points (file_path.cpp) run the same walk over a plan of one file (file_call.hpp).
//
// A file's index blocks are ordinary blocks of the image, the tree is at most three levels deep, and the number of
// index blocks at each level follows from the range alone (file_plan.hpp).  Level A of all the files of a call is one
// list, level B one list, level C one list and the data blocks one extent stream (files_plan.hpp), so the number of
// launches is that of one file.
//   plan    on the host: every file's span, its places in the call's arrays, the merged levels, per level a
//           table of (first entry, file) rows and one 128-byte record per file
//   upload  a batch only: the tables go through a page-locked buffer into the call's share of the scrub scratch, on
//           the caller's stream; the buffer returns to the cache once an event behind that copy has completed.  The
//           record of a single file travels in the kernel arguments instead
//   tree    per level A, B, C over the whole call: expand (files_walk.hip), ONE ppfs_ecc_decode_list_*,
//           merge (statuses, counts, file flags, the caller's level-major arrays)
//   blocks  per piece of fileplan::PIECE_BLOCKS merged file blocks, cut regardless of file boundaries:
//           expand; for a read also extents, ppfs_ecc_read_extents_* into the call's out, merge
//   write   the same plan under the stricter range rule (a write stays inside the file), per piece expand,
//           extents with pos pointing into the call's in, ppfs_ecc_write_extents_*, the write merge (`written`;
//           no payload byte is filled in); the batch's device form first refuses two ranges of one inode record
//           that share a file block
// The device forms queue all of it on the caller's stream and read nothing back; their scratch is the context's
// scrub scratch (scrub_path.cpp), so no call allocates or frees on the caller's stream.  The host forms run the
// same merged plan on the CPU around the *_host list and extent calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "file_call.hpp"
#include "kernels.hpp"
#include "list_call.hpp"

using namespace ppfs;
using namespace ppfs::fileplan;
using filesplan::FileRec;
using filesplan::Plan;
using filesplan::PlanView;
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
uint64_t entry_base(const PlanView& p, int level) { return level == LEVEL_A ? 0u : level == LEVEL_B ? p.total.tree[0] : p.total.tree[0] + p.total.tree[1]; }

// ------------------------------------------------------------------------------------------------------
// Device side
// ------------------------------------------------------------------------------------------------------
// A call's share of the context's scrub scratch: a batch's tables (the records, then the four row tables; a
// single file has none), the merged tree (a pointer, a decode status, an inherited status and a payload per
// slot; each level starts on a 16-entry boundary, so every level's payload and status pointers are 16-byte
// aligned and a context that decodes lists directly keeps doing so), a piece of merged file blocks (pointer,
// path status, extent, read or write status).
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
TableLayout table_layout(const PlanView& p)
{
    TableLayout t {};
    t.recs = 0;
    size_t at = round_up(p.nfiles * sizeof(FileRec), 256);
    for (int l = 0; l < filesplan::LEVELS; ++l) {
        t.rows[l] = at;
        at = round_up(at + (p.nrows[l] + 1) * sizeof(Row), 256);
    }
    t.bytes = at;
    return t;
}
// io: the call reads or writes, so a piece also has extents and statuses
size_t scratch_layout(const PlanView& p, size_t table_bytes, size_t ds, size_t piece, bool io, uint8_t* base, Scratch* s)
{
    const size_t slots = p.levels.slots;
    const size_t o_tidx = round_up(table_bytes, 256), o_tst = round_up(o_tidx + slots * 4, 256), o_tinh = round_up(o_tst + slots, 256),
                 o_tpay = round_up(o_tinh + slots, 256), o_idx = round_up(o_tpay + slots * ds + 16, 256),
                 o_path = round_up(o_idx + piece * 4, 256), o_ext = round_up(o_path + piece, 256),
                 o_rst = round_up(o_ext + (io ? piece * 16 : 0), 256),
                 bytes = round_up(o_rst + (io ? piece : 0), 256); // the codecs store statuses in whole 16-byte windows
    if (s)
        *s = Scratch { base, (uint32_t*)(base + o_tidx), base + o_tst, base + o_tinh, base + o_tpay, (uint32_t*)(base + o_idx),
            base + o_path, (ppfs_ecc_extent*)(base + o_ext), base + o_rst };
    return bytes;
}

// what a failed launch is reported under: the texts of the single-file calls and of the batch calls
struct Steps {
    const char *expand, *extents, *tree_merge, *blocks_merge, *read_merge, *write_merge, *written_init;
};
constexpr Steps kOneSteps { "file expand", "file extents", "file tree merge", "file blocks tally", "file read merge", "file write merge",
    "file written init" };
constexpr Steps kBatchSteps { "files expand", "files extents", "files merge", "files merge", "files merge", "files write merge",
    "files written init" };

struct DeviceWalk {
    const FileCall& a;
    void* stream;
    const PlanView& plan = a.plan;
    const size_t ds = a.c->data;
    const bool one = plan.one != nullptr;
    const Steps& step = one ? kOneSteps : kBatchSteps;
    Scratch x {};
    TableLayout tl {};
    hipStream_t s() const { return (hipStream_t)stream; }
    unsigned long long* counts() const { return (unsigned long long*)a.counts; }
    // who owns the entries of a launch at a level: the single file, or the batch's tables in the scratch
    ppfs_files_owner owner(int level) const
    {
        if (one)
            return ppfs_files_owner { nullptr, 0, nullptr, 0, plan.one };
        return ppfs_files_owner { x.tables + tl.recs, plan.nfiles, x.tables + tl.rows[level], plan.nrows[level], nullptr };
    }

    // the scratch (after a wait for its previous user); for a batch then the tables into it through a page-locked
    // buffer that outlives the copy
    int setup(size_t piece, bool io)
    {
        if (!one)
            tl = table_layout(plan);
        uint8_t* scratch = nullptr;
        int r = scrub_scratch(a.c, scratch_layout(plan, tl.bytes, ds, piece, io, nullptr, nullptr), s(), &scratch);
        if (r)
            return r;
        scratch_layout(plan, tl.bytes, ds, piece, io, scratch, &x);
        return one ? 0 : upload();
    }
    int upload()
    {
        return stage_upload(a.c, x.tables, tl.bytes, s(), "files", [&](uint8_t* pin) {
            std::memcpy(pin + tl.recs, plan.recs, plan.nfiles * sizeof(FileRec));
            for (int l = 0; l < filesplan::LEVELS; ++l)
                std::memcpy(pin + tl.rows[l], plan.rows[l], (plan.nrows[l] + 1) * sizeof(Row));
        });
    }
    int expand(int level, uint64_t e0, uint64_t n, uint32_t* pointer, uint8_t* inherited) const
    {
        const ppfs_files_owner who = owner(level);
        return check_hip(ppfs_files_expand_launch(&who, level, e0, n, ds, x.tpay, x.tst, x.tinh, plan.levels.slots, pointer, inherited, s()),
            step.expand);
    }
    int merge(int level, const uint8_t* path, const uint8_t* read, uint64_t e0, uint64_t n, uint8_t* status_out,
        const uint32_t* pointer_in, uint32_t* pointer_out, uint8_t* out, const char* what) const
    {
        const ppfs_files_owner who = owner(level);
        return check_hip(ppfs_files_merge_launch(&who, level, path, read, e0, n, status_out, pointer_in, pointer_out, out,
                             plan.total.bytes, ds, a.flags, counts(), s()),
            what);
    }
    // levels A, B, C of the whole call: each one list decode; the caller's arrays level-major (either may be null)
    int levels() const
    {
        int r = 0;
        for (int level = LEVEL_A; level <= LEVEL_C && !r; ++level) {
            const uint64_t n = plan.total.tree[level], at = plan.levels.base[level], to = entry_base(plan, level);
            if (n == 0)
                continue;
            (void)((r = expand(level, 0, n, x.tidx + at, x.tinh + at))
                || (r = ppfs_ecc_decode_list_device(a.c, a.image, blocks_seen(a.image_blocks), x.tidx + at, n, x.tpay + at * ds, x.tst + at,
                        a.wb, nullptr, stream))
                || (r = merge(level, x.tinh + at, x.tst + at, 0, n, a.tree_status ? a.tree_status + to : nullptr, x.tidx + at,
                        a.tree_index ? a.tree_index + to : nullptr, nullptr, step.tree_merge)));
        }
        return r;
    }
    // the merged file blocks [off, off + nb): expand, for a read or a write the extents and the extent call, the mode's merge
    int piece(uint64_t off, uint64_t nb) const
    {
        const bool io = a.mode != FileMode::blocks;
        uint32_t* idx = io ? x.idx : a.index ? a.index + off : nullptr;
        uint8_t* path = !io && a.path_status ? a.path_status + off : x.path;
        uint8_t* status = a.status ? a.status + off : nullptr;
        const ppfs_files_owner who = owner(LEVEL_DATA);
        int r = expand(LEVEL_DATA, off, nb, idx, path);
        if (!r && io)
            r = check_hip(ppfs_files_extents_launch(&who, idx, path, off, nb, ds, x.ext, s()), step.extents);
        if (r)
            return r;
        switch (a.mode) {
        case FileMode::blocks:
            return merge(LEVEL_DATA, path, nullptr, off, nb, nullptr, nullptr, nullptr, nullptr, step.blocks_merge);
        case FileMode::read:
            if ((r = ppfs_ecc_read_extents_device(a.c, a.image, a.image_blocks, x.ext, nb, a.out, plan.total.bytes, x.rst, a.wb, stream)))
                return r;
            return merge(LEVEL_DATA, path, x.rst, off, nb, status, nullptr, nullptr, a.out, step.read_merge);
        default:
            if ((r = ppfs_ecc_write_extents_device(a.c, a.in, plan.total.bytes, a.image, a.image_blocks, x.ext, nb, x.rst, stream)))
                return r;
            return check_hip(ppfs_files_write_merge_launch(&who, path, x.rst, off, nb, status, ds, a.flags,
                                 (unsigned long long*)a.written, counts(), s()),
                step.write_merge);
        }
    }
};

// what the batch's device forms do before the walk: refuse a capture, clear the counts and the flags
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

// page-locked buffers of earlier staged calls whose copy has completed go back to the cache
static void reap_stages(ppfs_ecc_ctx* c)
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

int ppfs::stage_upload(ppfs_ecc_ctx* c, uint8_t* d_dst, size_t bytes, hipStream_t s, const char* who, const std::function<void(uint8_t*)>& fill)
{
    reap_stages(c);
    size_t cap = 4096; // few distinct sizes, so that the cache of page-locked buffers hits
    while (cap < bytes)
        cap *= 2;
    uint8_t* pin = nullptr;
    if (pin_alloc((void**)&pin, cap, kPinStage) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PPFS_ECC_ENOMEM, (std::string(who) + ": page-locked staging of the tables").c_str());
    }
    fill(pin);
    hipError_t e = dma_async(d_dst, pin, bytes, hipMemcpyHostToDevice, s);
    hipEvent_t done = nullptr;
    if (e == hipSuccess && (e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) == hipSuccess
        && (e = hipEventRecord(done, s)) == hipSuccess) {
        c->files_stage.push_back(ppfs_ecc_ctx::FilesStage { pin, cap, done });
        return 0;
    }
    // nothing to tell the copy's end by: drain the stream, then the buffer is free
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    if (done)
        (void)hipEventDestroy(done);
    pin_free(pin, cap, kPinStage);
    return fail(PPFS_ECC_EHIP, (std::string(who) + ": table upload").c_str(), e);
}

int ppfs::file_call_device(const FileCall& a, void* stream, const char* queued)
{
    const uint64_t nblocks = a.plan.total.blocks;
    const size_t piece = std::min<uint64_t>(nblocks, PIECE_BLOCKS);
    const bool io = a.mode != FileMode::blocks;
    DeviceWalk w { a, stream };
    int r = w.setup(piece, io);
    if (r)
        return r;
    if (a.mode == FileMode::write) {
        const ppfs_files_owner who = w.owner(LEVEL_DATA);
        r = check_hip(ppfs_files_written_init_launch(&who, (unsigned long long*)a.written, w.s()), w.step.written_init);
    }
    if (!r)
        r = w.levels();
    if (io || a.index || a.path_status || a.counts || a.flags)
        for (uint64_t off = 0; off < nblocks && !r; off += piece)
            r = w.piece(off, std::min<uint64_t>(piece, nblocks - off));
    scrub_scratch_used(a.c, w.s());
    return call_queued(a.c, r, nblocks, stream, queued);
}

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
    if ((r = device_begin((hipStream_t)stream, nfiles, d_file_flags, d_counts)) || plan.total.blocks == 0)
        return r;
    FileCall a { c, d_image, image_blocks, plan.view(), FileMode::blocks, write_back ? 1 : 0 };
    a.index = d_index;
    a.path_status = d_path_status;
    a.tree_index = d_tree_index;
    a.tree_status = d_tree_status;
    a.flags = d_file_flags;
    a.counts = d_counts;
    return file_call_device(a, stream, "files blocks (async)");
}

extern "C" int ppfs_ecc_read_files_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* files,
    const ppfs_ecc_file_range* ranges, size_t nfiles, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, uint32_t* d_file_flags,
    ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Plan plan;
    int r = batch_args(c, files, ranges, nfiles, "read files", plan);
    if (r || (r = read_args(c, d_image, plan, d_out, out_bytes, d_file_flags, d_counts, "read files")))
        return r;
    if ((r = device_begin((hipStream_t)stream, nfiles, d_file_flags, d_counts)) || plan.total.blocks == 0)
        return r;
    FileCall a { c, d_image, image_blocks, plan.view(), FileMode::read, write_back ? 1 : 0 };
    a.out = d_out;
    a.status = d_status;
    a.flags = d_file_flags;
    a.counts = d_counts;
    return file_call_device(a, stream, "read files (async)");
}

// FileIO::writeFile over an existing range (file_io.cpp:46-104) for every file of a batch
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
    if (plan.total.blocks == 0) { // every range is empty: nothing is written, of nothing
        if (d_written && nfiles)
            HIP_TRY(hipMemsetAsync(d_written, 0, nfiles * sizeof(uint64_t), s), "files written clear");
        return 0;
    }
    FileCall a { c, d_image, image_blocks, plan.view(), FileMode::write, write_back ? 1 : 0 };
    a.in = d_in;
    a.status = d_status;
    a.flags = d_file_flags;
    a.written = d_written;
    a.counts = d_counts;
    return file_call_device(a, stream, "write files (async)");
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
    const FileCall& a;
    const PlanView& plan = a.plan;
    const size_t ds = a.c->data;
    std::vector<uint32_t> tidx {};
    std::vector<uint8_t> tst {}, tinh {}, tpay {};

    HostMem mem() const { return HostMem { tpay.data(), tst.data(), tinh.data() }; }
    void note(uint32_t file, uint32_t st, bool tree) const
    {
        const int slot = count_slot(st);
        if (a.counts && slot >= 0)
            ++(&a.counts->ok)[(tree ? SLOT_INDEX : SLOT_FILE) + slot];
        if (a.flags)
            a.flags[file] |= filesplan::flag_of(st) << (tree ? filesplan::FLAG_TREE_SHIFT : 0u);
    }
    // fn(file, k, merged entry) for every entry of a level, in merged order
    template <class Fn>
    void each(int level, Fn fn) const
    {
        const Row* rows = plan.rows[level];
        for (size_t r = 0; r < plan.nrows[level]; ++r)
            for (uint64_t e = rows[r].first; e < rows[r + 1].first; ++e)
                fn(rows[r].file, e - rows[r].first, e);
    }
    int levels()
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
            const int r = ppfs_ecc_decode_list_host(a.c, a.image, blocks_seen(a.image_blocks), tidx.data() + at, n, tpay.data() + at * ds,
                tst.data() + at, a.wb, nullptr);
            if (r)
                return r;
            each(level, [&](uint32_t f, uint64_t, uint64_t e) {
                const uint8_t st = tinh[at + e] ? tinh[at + e] : tst[at + e];
                if (a.tree_index)
                    a.tree_index[to + e] = tidx[at + e];
                if (a.tree_status)
                    a.tree_status[to + e] = st;
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

int ppfs::file_call_host(const FileCall& a)
{
    const PlanView& plan = a.plan;
    const uint64_t nblocks = plan.total.blocks;
    HostBatch w { a };
    int r = w.levels();
    if (r)
        return r;
    const HostMem m = w.mem();
    if (a.mode == FileMode::blocks) {
        w.each(LEVEL_DATA, [&](uint32_t f, uint64_t k, uint64_t e) {
            const Expanded x = filesplan::expand_entry(plan.recs[f], LEVEL_DATA, k, w.ds, m);
            if (a.index)
                a.index[e] = x.pointer;
            if (a.path_status)
                a.path_status[e] = x.inherited;
            w.note(f, x.inherited, false);
        });
        return 0;
    }
    // a read or a write: the extents, the extent call, then path status over its status
    std::vector<ppfs_ecc_extent> ext(nblocks);
    std::vector<uint8_t> path(nblocks), st(nblocks);
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t k, uint64_t e) {
        const FileRec& rec = plan.recs[f];
        const Expanded x = filesplan::expand_entry(rec, LEVEL_DATA, k, w.ds, m);
        const Extent at = extent_of(k, rec.off0, rec.bytes, w.ds);
        path[e] = x.inherited;
        ext[e] = ppfs_ecc_extent { rec.out_pos + at.pos, x.inherited ? NO_BLOCK : x.pointer, (uint16_t)at.offset, (uint16_t)at.length };
    });
    const bool read = a.mode == FileMode::read;
    if ((r = read ? ppfs_ecc_read_extents_host(a.c, a.image, a.image_blocks, ext.data(), nblocks, a.out, plan.total.bytes, st.data(), a.wb)
                  : ppfs_ecc_write_extents_host(a.c, a.in, plan.total.bytes, a.image, a.image_blocks, ext.data(), nblocks, st.data())))
        return r;
    w.each(LEVEL_DATA, [&](uint32_t f, uint64_t, uint64_t e) {
        const uint8_t fin = path[e] ? path[e] : st[e];
        if (a.status)
            a.status[e] = fin;
        if (read && path[e] == STATUS_FAILED) // the zero fill under a failed index block
            std::memset(a.out + ext[e].pos, 0, ext[e].length);
        if (!read && a.written && (fin == STATUS_FAILED || fin == STATUS_OUT)) // lowered to the first failing block's position
            a.written[f] = std::min<uint64_t>(a.written[f], ext[e].pos - plan.recs[f].out_pos);
        w.note(f, fin, false);
    });
    return 0;
}

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
    FileCall a { c, image, image_blocks, plan.view(), FileMode::blocks, write_back ? 1 : 0 };
    a.index = index;
    a.path_status = path_status;
    a.tree_index = tree_index;
    a.tree_status = tree_status;
    a.flags = file_flags;
    a.counts = counts;
    return file_call_host(a);
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
    if (plan.total.blocks == 0)
        return 0;
    FileCall a { c, image, image_blocks, plan.view(), FileMode::read, write_back ? 1 : 0 };
    a.out = out;
    a.status = status;
    a.flags = file_flags;
    a.counts = counts;
    return file_call_host(a);
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
    if (plan.total.blocks == 0)
        return 0;
    FileCall a { c, image, image_blocks, plan.view(), FileMode::write, write_back ? 1 : 0 };
    a.in = in;
    a.status = status;
    a.flags = file_flags;
    a.written = written;
    a.counts = counts;
    return file_call_host(a);
}
