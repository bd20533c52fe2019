// files_walk.hip -- the kernels of the file walk (files_path.cpp; include/ppfs_ecc.h ppfs_ecc_file_blocks_*,
// ppfs_ecc_read_file_*, ppfs_ecc_write_file_* and their ppfs_ecc_files_* batch forms).
//
// A file's index-block tree is at most three levels deep, and how many index blocks a walk over a range of its
// file blocks visits at each level follows from the range alone (file_plan.hpp).  Every level of all the files of
// a call is one merged list (files_plan.hpp), so the walk is one list decode per level with an expansion in
// between, all queued, nothing read back:
//   files_expand_kernel   one merged level (or a piece of the merged file blocks): the file that owns the
//                         lane's entry, its record, the entry's number k within that file, then fileplan's
//                         expansion against the merged scratch
//   files_extents_kernel  a piece of merged file blocks: pos = the file's out_pos + its extent's pos
//   files_merge_kernel    path status over read status, zero fill under a failed index block within the
//                         file's own range, the counts, the file flags; for a level of the tree also its
//                         pointers and statuses into the caller's level-major arrays
// and of the writes, which reuse the expansion and the extents:
//   files_written_init_kernel   written[f] = file f's bytes, one lane per file
//   files_write_merge_kernel    path status over write status, the counts, the file flags, written[file]
//                               lowered to the first failing block's position; no payload byte is touched
// One lane per merged entry, 256 lanes a workgroup; consecutive lanes store consecutive elements.
//
// Each kernel is a template on who owns an entry:
//   OneFile  the call is about one file, whose record and Tree travel by value in the kernel arguments: entry e
//            is entry k = e of file 0; no table, no search, no global read, no Tree rebuilt per lane
//   Batch    the batch's records and the level's row table in device memory: every lane binary-searches the
//            table (owner_of).  The other form that was built and measured -- the workgroup loads the at most
//            256 rows of its 256 entries into LDS and the lanes search there -- was no faster on either
//            workload of DESIGN.md section 4.11 and lives in tools/ablations/files_lookup_lds.hpp
//            (tools/build_alt.sh files_lds -DPPFS_FILES_LOOKUP_LDS=1).
// Nothing read from the tables is used unchecked: a file number is compared with nfiles, an entry number k
// with the file's level count, and every scratch position and out position with its array's extent.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "files_plan.hpp"
#include "kernels.hpp"
#include "status_tally.hpp"
#include <stdint.h>

namespace ppfs {

using filesplan::FileRec;
using filesplan::OneRec;
using filesplan::Row;

// the records of the batch and the row table of the level a launch works on (rows: without the sentinel)
struct FilesTables {
    const FileRec* recs;
    uint64_t nfiles;
    const Row* rows;
    uint64_t nrows;
};

// the merged tree scratch
struct FilesMem {
    const uint8_t* payload; // slots * ds bytes
    uint64_t payload_bytes;
    const uint8_t* st;  // decode statuses, one per slot
    const uint8_t* inh; // inherited path statuses, one per slot
    uint64_t slots;
    __device__ uint32_t status(uint64_t p) const { return PPFS_DBG_OK(st + p, 1, st, slots) && p < slots ? st[p] : 9u; }
    __device__ uint32_t inherited(uint64_t p) const { return PPFS_DBG_OK(inh + p, 1, inh, slots) && p < slots ? inh[p] : 9u; }
    // a byte, never a dword: ds is rarely a multiple of 4 and the last entry of the last payload ends
    // where the scratch's payload area does
    __device__ uint32_t payload_byte(uint64_t at) const
    {
        return PPFS_DBG_OK(payload + at, 1, payload, payload_bytes) && at < payload_bytes ? payload[at] : 0xFFu;
    }
};

struct Owner {
    uint32_t file;
    uint64_t k; // the entry's number within its file's level
    bool ok;
};

#ifdef PPFS_FILES_LOOKUP_LDS
#include "files_lookup_lds.hpp"
#else
// The file that owns merged entry e.  [w0, w0 + wn) are the entries of this pass of the workgroup, 1 <= wn <= 256
// (what a workgroup-wide form needs); want: this lane needs an answer.  kOwnerAllLanes: every lane of the
// workgroup must call, wanted or not.
constexpr bool kOwnerAllLanes = false;
__device__ inline Owner owner_of(const FilesTables& tb, uint64_t w0, uint64_t wn, uint64_t e, bool want)
{
    Row r { 0, 0xFFFFFFFFu, 0 };
    if (want) {
        const uint64_t at = filesplan::row_of(tb.rows, tb.nrows, e);
        if (at < tb.nrows && PPFS_DBG_OK(tb.rows + at, 16, tb.rows, tb.nrows * 16))
            r = tb.rows[at];
    }
    Owner o;
    o.file = r.file;
    o.ok = want && r.file < tb.nfiles && r.first <= e && PPFS_DBG_OK(tb.recs + r.file, 128, tb.recs, tb.nfiles * 128);
    o.k = e - r.first;
    return o;
}
#endif

// The two owners.  owner(w0, wn, e, want) as owner_of; rec(f): the record of a file that owner() or has() found;
// expand(f, ...): filesplan::expand_entry of that file;
// has(f): file f is one of the call's (written_init's lanes); continues(file, stopped, lane): see there; kAllLanes: owner_of's kOwnerAllLanes.
struct OneFile {
    OneRec one;     // the record and the Tree of its range, built once on the host
    uint64_t count; // the entries of the level the launch works on
    static constexpr bool kAllLanes = false;
    static constexpr uint32_t kInitLanes = 64; // written_init's workgroup: one wave for the one word
    __device__ uint64_t nfiles() const { return 1u; }
    __device__ bool has(uint64_t f) const { return f == 0u; }
    __device__ const FileRec& rec(uint32_t) const { return one.rec; }
    template <class Mem>
    __device__ fileplan::Expanded expand(uint32_t, int level, uint64_t k, uint64_t ds, const Mem& mem) const
    {
        return filesplan::expand_entry(one.rec, one.tree, level, k, ds, mem);
    }
    __device__ Owner owner(uint64_t, uint64_t, uint64_t e, bool want) const { return Owner { 0u, e, want && e < count }; }
    // every lane of the wave: an earlier lane of `stopped` (the ballot of the lanes that lower written[file]) lowers it
    // to a position no greater than this lane's.  One file: any earlier lane, so only the wave's first one is left
    __device__ bool continues(uint32_t, unsigned long long stopped, uint32_t lane) const { return (stopped & ((1ull << lane) - 1ull)) != 0; }
};
struct Batch {
    FilesTables tb;
    static constexpr bool kAllLanes = kOwnerAllLanes;
    static constexpr uint32_t kInitLanes = 256;
    __device__ uint64_t nfiles() const { return tb.nfiles; }
    __device__ bool has(uint64_t f) const { return f < tb.nfiles && PPFS_DBG_OK(tb.recs + f, 128, tb.recs, tb.nfiles * 128); }
    __device__ const FileRec& rec(uint32_t f) const { return tb.recs[f]; }
    template <class Mem>
    __device__ fileplan::Expanded expand(uint32_t f, int level, uint64_t k, uint64_t ds, const Mem& mem) const
    {
        return filesplan::expand_entry(tb.recs[f], level, k, ds, mem); // the Tree rebuilt from the record
    }
    __device__ Owner owner(uint64_t w0, uint64_t wn, uint64_t e, bool want) const { return owner_of(tb, w0, wn, e, want); }
    // a batch: the lane before this one, when it has the same file, so the first lane of every run of one file is left.
    // The shuffle runs in every lane, before anything is decided by it
    __device__ bool continues(uint32_t file, unsigned long long stopped, uint32_t lane) const
    {
        const uint32_t file_before = (uint32_t)__shfl_up((int)file, 1);
        return lane > 0u && ((stopped >> (lane - 1u)) & 1ull) && file_before == file;
    }
};

// merged entries [e0, e0 + n) of a level: pointer[i] and inherited[i] for entry e0 + i (either may be null)
template <class Who>
__global__ __launch_bounds__(256) void files_expand_kernel(Who who, FilesMem mem, int level, uint64_t e0, uint64_t n,
    uint64_t ds, uint32_t* __restrict__ pointer, uint8_t* __restrict__ inherited)
{
    const uint64_t w0 = (uint64_t)blockIdx.x * 256u, i = w0 + threadIdx.x;
    if (w0 >= n)
        return;
    const bool live = i < n;
    const Owner o = who.owner(e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, live);
    if (!live)
        return;
    fileplan::Expanded x { fileplan::NO_BLOCK, fileplan::STATUS_OUT };
    if (o.ok)
        x = who.expand(o.file, level, o.k, ds, mem);
    if (pointer && PPFS_DBG_OK(pointer + i, 4, pointer, n * 4))
        pointer[i] = x.pointer;
    if (inherited && PPFS_DBG_OK(inherited + i, 1, inherited, n))
        inherited[i] = x.inherited;
}

// ext[i] = the read of merged file block e0 + i: the resolved block, or NO_BLOCK where the path failed, at
// its file's place in the batch's out
template <class Who>
__global__ __launch_bounds__(256) void files_extents_kernel(Who who, const uint32_t* __restrict__ pointer,
    const uint8_t* __restrict__ path, uint64_t e0, uint64_t n, uint64_t ds, ppfs_ecc_extent* __restrict__ ext)
{
    const uint64_t w0 = (uint64_t)blockIdx.x * 256u, i = w0 + threadIdx.x;
    if (w0 >= n)
        return;
    const bool live = i < n && PPFS_DBG_OK(pointer + i, 4, pointer, n * 4) && PPFS_DBG_OK(path + i, 1, path, n);
    const Owner o = who.owner(e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, live);
    if (!live)
        return;
    ppfs_ecc_extent e;
    e.pos = 0;
    e.block = fileplan::NO_BLOCK;
    e.offset = e.length = 0;
    if (o.ok) {
        const FileRec& rec = who.rec(o.file);
        const fileplan::Extent x = fileplan::extent_of(o.k, rec.off0, rec.bytes, ds);
        e.pos = rec.out_pos + x.pos;
        e.block = path[i] ? fileplan::NO_BLOCK : pointer[i];
        e.offset = (uint16_t)x.offset;
        e.length = (uint16_t)x.length;
    }
    if (PPFS_DBG_OK(ext + i, 16, ext, n * 16))
        ext[i] = e;
}

// Merged entries e0 + i, i < n: the final status is path[i] where that is non-zero, else read[i] (null: 0).
//   status_out (may be null)            the final statuses
//   pointer_in / pointer_out (may be null, together)  a level's pointers into the caller's array
//   out (may be null)                   the batch's packed buffer of out_bytes bytes: the range of a block with
//                                       path status 5 is zero-filled within its file's range
//   flags (may be null)                 flags[file] |= filesplan::flag_of(final) << flag_shift, one atomicOr per
//                                       lane whose status is non-zero; zeroed on the stream before
//   counts (may be null)                counts[slot0 + fileplan::count_slot(final)] grows by one (status_tally.hpp)
template <class Who>
__global__ __launch_bounds__(256) void files_merge_kernel(Who who, const uint8_t* __restrict__ path,
    const uint8_t* __restrict__ read, uint64_t e0, uint64_t n, uint8_t* __restrict__ status_out,
    const uint32_t* __restrict__ pointer_in, uint32_t* __restrict__ pointer_out, uint8_t* __restrict__ out, uint64_t out_bytes,
    uint64_t ds, uint32_t* __restrict__ flags, uint32_t flag_shift, unsigned long long* __restrict__ counts, int slot0)
{
    uint32_t c[4] = { 0, 0, 0, 0 };
    for (uint64_t w0 = (uint64_t)blockIdx.x * 256u; w0 < n; w0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = w0 + threadIdx.x;
        const bool live = i < n && PPFS_DBG_OK(path + i, 1, path, n);
        uint32_t p = 0, s = 0;
        int slot = -1;
        if (live) {
            p = path[i];
            s = p ? p : (read && PPFS_DBG_OK(read + i, 1, read, n) ? read[i] : 0u);
            slot = fileplan::count_slot(s);
            if (status_out && PPFS_DBG_OK(status_out + i, 1, status_out, n))
                status_out[i] = (uint8_t)s;
            if (pointer_out && PPFS_DBG_OK(pointer_in + i, 4, pointer_in, n * 4) && PPFS_DBG_OK(pointer_out + i, 4, pointer_out, n * 4))
                pointer_out[i] = pointer_in[i];
        }
        const bool fill = out && p == fileplan::STATUS_FAILED, want = live && ((flags && s) || fill);
        if (Who::kAllLanes || want) {
            const Owner o = who.owner(e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, want);
            if (o.ok) {
                const uint32_t bit = filesplan::flag_of(s) << flag_shift;
                if (flags && bit && PPFS_DBG_OK(flags + o.file, 4, flags, who.nfiles() * 4))
                    atomicOr(flags + o.file, bit);
                if (fill) {
                    const FileRec& rec = who.rec(o.file);
                    const fileplan::Extent x = fileplan::extent_of(o.k, rec.off0, rec.bytes, ds);
                    const uint64_t at = rec.out_pos + x.pos;
                    for (uint32_t b = 0; b < x.length; ++b)
                        if (x.pos + b < rec.bytes && at + b < out_bytes && PPFS_DBG_OK(out + at + b, 1, out, out_bytes))
                            out[at + b] = 0;
                }
            }
        }
        tally_add(c, slot);
    }
    tally_flush(c, counts, slot0, 4);
}

// written[f] = file f's bytes, one lane per file: what a write reports for a file none of whose blocks fails
// (the write merge lowers it)
template <class Who>
__global__ __launch_bounds__(256) void files_written_init_kernel(Who who, unsigned long long* __restrict__ written)
{
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (who.has(f) && PPFS_DBG_OK(written + f, 8, written, who.nfiles() * 8))
        written[f] = who.rec((uint32_t)f).bytes;
}

// The merge of a WRITE over the merged file blocks e0 + i, i < n: the final status is path[i] where that
// is non-zero, else wst[i], the write's.  It reads and writes no payload byte.
//   status_out (may be null)   the final statuses
//   flags (may be null)        as files_merge_kernel's, the data bits
//   written (may be null)      written[file] lowered to the block's position within its file's bytes for a final
//                              status 5 or 9: a 64-bit atomicMin from the first lane of every run of such lanes of
//                              one file within a wave (positions grow along a file's entries)
//   counts (may be null)       the tally into the file half
template <class Who>
__global__ __launch_bounds__(256) void files_write_merge_kernel(Who who, const uint8_t* __restrict__ path,
    const uint8_t* __restrict__ wst, uint64_t e0, uint64_t n, uint8_t* __restrict__ status_out, uint64_t ds,
    uint32_t* __restrict__ flags, unsigned long long* __restrict__ written, unsigned long long* __restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t c[4] = { 0, 0, 0, 0 };
    for (uint64_t w0 = (uint64_t)blockIdx.x * 256u; w0 < n; w0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = w0 + threadIdx.x;
        const bool live = i < n && PPFS_DBG_OK(path + i, 1, path, n);
        uint32_t s = 0;
        int slot = -1;
        if (live) {
            const uint32_t p = path[i];
            s = p ? p : (wst && PPFS_DBG_OK(wst + i, 1, wst, n) ? wst[i] : 0u);
            slot = fileplan::count_slot(s);
            if (status_out && PPFS_DBG_OK(status_out + i, 1, status_out, n))
                status_out[i] = (uint8_t)s;
        }
        const bool bad = slot == 2 || slot == 3, want = live && ((flags && s) || (written && bad));
        Owner o;
        o.file = 0xFFFFFFFFu;
        o.k = 0;
        o.ok = false;
        if (Who::kAllLanes || want)
            o = who.owner(e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, want);
        const bool stop = o.ok && written && bad;
        const unsigned long long stopped = __builtin_amdgcn_ballot_w64(stop);
        const bool continues = who.continues(o.file, stopped, lane);
        if (o.ok) {
            const uint32_t bit = filesplan::flag_of(s);
            if (flags && bit && PPFS_DBG_OK(flags + o.file, 4, flags, who.nfiles() * 4))
                atomicOr(flags + o.file, bit);
            if (stop && !continues && PPFS_DBG_OK(written + o.file, 8, written, who.nfiles() * 8)) {
                const FileRec& rec = who.rec(o.file);
                const uint64_t pos = fileplan::extent_of(o.k, rec.off0, rec.bytes, ds).pos;
                atomicMin(written + o.file, (unsigned long long)(pos < rec.bytes ? pos : rec.bytes));
            }
        }
        tally_add(c, slot);
    }
    tally_flush(c, counts, fileplan::SLOT_FILE, 4);
}

static bool grid_of(uint64_t n, uint32_t& grid)
{
    const uint64_t g = (n + 255u) / 256u;
    grid = (uint32_t)g;
    return g <= 0x7FFFFFFFull;
}
// The launch's owner out of the ABI's ppfs_files_owner, handed to fn: the tables checked, or the one file's record
// copied with its entries at `level`
template <class Fn>
static hipError_t with_owner(const ppfs_files_owner* w, int level, Fn fn)
{
    if (!w || level < fileplan::LEVEL_A || level > fileplan::LEVEL_DATA)
        return hipErrorInvalidValue;
    if (w->one) {
        const OneRec& one = *(const OneRec*)w->one;
        return fn(OneFile { one, fileplan::level_count(one.tree, level) });
    }
    if (!w->recs || !w->rows || (((uintptr_t)w->recs | (uintptr_t)w->rows) & 7u) || w->nfiles < 1 || w->nfiles >= 0xFFFFFFFFull
        || w->nrows < 1 || w->nrows > w->nfiles)
        return hipErrorInvalidValue;
    return fn(Batch { FilesTables { (const FileRec*)w->recs, w->nfiles, (const Row*)w->rows, w->nrows } });
}
// the merges: grid-stride, at most 2,048 workgroups
static uint32_t merge_grid(uint64_t n)
{
    const uint64_t want = (n + 255u) / 256u;
    return (uint32_t)(want < 2048u ? want : 2048u);
}

} // namespace ppfs

using namespace ppfs;

extern "C" hipError_t ppfs_files_expand_launch(const ppfs_files_owner* owner, int level, uint64_t e0, uint64_t n, uint64_t ds,
    const uint8_t* payload, const uint8_t* st, const uint8_t* inh, uint64_t slots, uint32_t* pointer, uint8_t* inherited,
    hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (((uintptr_t)pointer & 3u) || !grid_of(n, grid))
        return hipErrorInvalidValue;
    const FilesMem mem { payload, slots * ds, st, inh, slots };
    return with_owner(owner, level, [&](auto who) {
        hipLaunchKernelGGL(files_expand_kernel<decltype(who)>, dim3(grid), dim3(256), 0, s, who, mem, level, e0, n, ds, pointer,
            inherited);
        return hipGetLastError();
    });
}

extern "C" hipError_t ppfs_files_extents_launch(const ppfs_files_owner* owner, const uint32_t* pointer, const uint8_t* path,
    uint64_t e0, uint64_t n, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (!pointer || !path || !ext || ds == 0 || ds > 0xFFFFu || ((uintptr_t)pointer & 3u) || ((uintptr_t)ext & 7u) || !grid_of(n, grid))
        return hipErrorInvalidValue;
    return with_owner(owner, fileplan::LEVEL_DATA, [&](auto who) {
        hipLaunchKernelGGL(files_extents_kernel<decltype(who)>, dim3(grid), dim3(256), 0, s, who, pointer, path, e0, n, ds, ext);
        return hipGetLastError();
    });
}

extern "C" hipError_t ppfs_files_merge_launch(const ppfs_files_owner* owner, int level, const uint8_t* path, const uint8_t* read,
    uint64_t e0, uint64_t n, uint8_t* status_out, const uint32_t* pointer_in, uint32_t* pointer_out, uint8_t* out,
    uint64_t out_bytes, uint64_t ds, uint32_t* flags, unsigned long long* counts, hipStream_t s)
{
    if (n == 0 || (!status_out && !pointer_out && !out && !counts && !flags))
        return hipSuccess;
    if (!path || (pointer_out && !pointer_in) || (((uintptr_t)pointer_in | (uintptr_t)pointer_out | (uintptr_t)flags) & 3u)
        || ((uintptr_t)counts & 7u) || (out && ds == 0))
        return hipErrorInvalidValue;
    const bool tree = level != fileplan::LEVEL_DATA;
    return with_owner(owner, level, [&](auto who) {
        hipLaunchKernelGGL(files_merge_kernel<decltype(who)>, dim3(merge_grid(n)), dim3(256), 0, s, who, path, read, e0, n, status_out,
            pointer_out ? pointer_in : nullptr, pointer_out, out, out_bytes, ds, flags, tree ? filesplan::FLAG_TREE_SHIFT : 0u, counts,
            tree ? fileplan::SLOT_INDEX : fileplan::SLOT_FILE);
        return hipGetLastError();
    });
}

extern "C" hipError_t ppfs_files_written_init_launch(const ppfs_files_owner* owner, unsigned long long* written, hipStream_t s)
{
    uint32_t grid;
    const uint64_t nfiles = owner ? (owner->one ? 1u : owner->nfiles) : 0u;
    if (!written || nfiles == 0)
        return hipSuccess;
    if (((uintptr_t)written & 7u) || !grid_of(nfiles, grid))
        return hipErrorInvalidValue;
    return with_owner(owner, fileplan::LEVEL_DATA, [&](auto who) {
        hipLaunchKernelGGL(files_written_init_kernel<decltype(who)>, dim3(grid), dim3(decltype(who)::kInitLanes), 0, s, who, written);
        return hipGetLastError();
    });
}

extern "C" hipError_t ppfs_files_write_merge_launch(const ppfs_files_owner* owner, const uint8_t* path, const uint8_t* wst, uint64_t e0,
    uint64_t n, uint8_t* status_out, uint64_t ds, uint32_t* flags, unsigned long long* written, unsigned long long* counts,
    hipStream_t s)
{
    if (n == 0 || (!status_out && !flags && !written && !counts))
        return hipSuccess;
    if (!path || ((uintptr_t)flags & 3u) || (((uintptr_t)written | (uintptr_t)counts) & 7u) || ds == 0)
        return hipErrorInvalidValue;
    return with_owner(owner, fileplan::LEVEL_DATA, [&](auto who) {
        hipLaunchKernelGGL(files_write_merge_kernel<decltype(who)>, dim3(merge_grid(n)), dim3(256), 0, s, who, path, wst, e0, n,
            status_out, ds, flags, written, counts);
        return hipGetLastError();
    });
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_files_faults)
