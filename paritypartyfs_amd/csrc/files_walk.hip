// files_walk.hip -- the kernels of the read-only walk over a batch of files (files_path.cpp; include/ppfs_ecc.h
// ppfs_ecc_files_blocks_*, ppfs_ecc_read_files_*).  They are file_walk.hip's three kernels in batch form:
// every level of all the files is one merged list (files_plan.hpp), and a lane first finds the file that
// owns its merged entry.
//   files_expand_kernel   one merged level (or a piece of the merged file blocks): the lane's row, its
//                         file's record, its entry k of that file, then fileplan's expansion against the
//                         merged scratch
//   files_extents_kernel  a piece of merged file blocks: pos = the file's out_pos + its extent's pos
//   files_merge_kernel    path status over read status, zero fill under a failed index block within the
//                         file's own range, the counts, the file flags; for a level of the tree also its
//                         pointers and statuses into the caller's level-major arrays
// and of the batch write (ppfs_ecc_write_files_*), which reuses the expansion and the extents:
//   files_written_init_kernel   written[f] = file f's bytes, one lane per file
//   files_write_merge_kernel    path status over write status, the counts, the file flags, written[file]
//                               lowered to the first failing block's position; no payload byte is touched
// One lane per merged entry, 256 lanes a workgroup; consecutive lanes store consecutive elements.
//
// The row lookup: every lane binary-searches the level's table in global memory (owner_of).  The other form
// that was built and measured -- the workgroup loads the at most 256 rows of its 256 entries into LDS and the
// lanes search there -- was no faster on either workload of DESIGN.md section 4.11 and lives in
// tools/ablations/files_lookup_lds.hpp (tools/build_alt.sh files_lds -DPPFS_FILES_LOOKUP_LDS=1).
// Nothing read from the tables is used unchecked: a file number is compared with nfiles, an entry number k
// with the file's level count, and every scratch position and out position with its array's extent.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "files_plan.hpp"
#include "kernels.hpp"
#include <stdint.h>

namespace ppfs {

using filesplan::FileRec;
using filesplan::Row;

// the records of the batch and the row table of the level a launch works on (rows: without the sentinel)
struct FilesTables {
    const FileRec* recs;
    uint64_t nfiles;
    const Row* rows;
    uint64_t nrows;
};

// the merged tree scratch, as file_walk.hip's FileSrc reads a single file's
struct FilesMem {
    const uint8_t* payload; // slots * ds bytes
    uint64_t payload_bytes;
    const uint8_t* st;  // decode statuses, one per slot
    const uint8_t* inh; // inherited path statuses, one per slot
    uint64_t slots;
    __device__ uint32_t status(uint64_t p) const { return PPFS_DBG_OK(st + p, 1, st, slots) && p < slots ? st[p] : 9u; }
    __device__ uint32_t inherited(uint64_t p) const { return PPFS_DBG_OK(inh + p, 1, inh, slots) && p < slots ? inh[p] : 9u; }
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

// merged entries [e0, e0 + n) of a level: pointer[i] and inherited[i] for entry e0 + i (either may be null)
__global__ __launch_bounds__(256) void files_expand_kernel(FilesTables tb, FilesMem mem, int level, uint64_t e0, uint64_t n,
    uint64_t ds, uint32_t* __restrict__ pointer, uint8_t* __restrict__ inherited)
{
    const uint64_t w0 = (uint64_t)blockIdx.x * 256u, i = w0 + threadIdx.x;
    if (w0 >= n)
        return;
    const bool live = i < n;
    const Owner o = owner_of(tb, e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, live);
    if (!live)
        return;
    fileplan::Expanded x { fileplan::NO_BLOCK, fileplan::STATUS_OUT };
    if (o.ok)
        x = filesplan::expand_entry(tb.recs[o.file], level, o.k, ds, mem);
    if (pointer && PPFS_DBG_OK(pointer + i, 4, pointer, n * 4))
        pointer[i] = x.pointer;
    if (inherited && PPFS_DBG_OK(inherited + i, 1, inherited, n))
        inherited[i] = x.inherited;
}

// ext[i] = the read of merged file block e0 + i: the resolved block, or NO_BLOCK where the path failed, at
// its file's place in the batch's out
__global__ __launch_bounds__(256) void files_extents_kernel(FilesTables tb, const uint32_t* __restrict__ pointer,
    const uint8_t* __restrict__ path, uint64_t e0, uint64_t n, uint64_t ds, ppfs_ecc_extent* __restrict__ ext)
{
    const uint64_t w0 = (uint64_t)blockIdx.x * 256u, i = w0 + threadIdx.x;
    if (w0 >= n)
        return;
    const bool live = i < n && PPFS_DBG_OK(pointer + i, 4, pointer, n * 4) && PPFS_DBG_OK(path + i, 1, path, n);
    const Owner o = owner_of(tb, e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, live);
    if (!live)
        return;
    ppfs_ecc_extent e;
    e.pos = 0;
    e.block = fileplan::NO_BLOCK;
    e.offset = e.length = 0;
    if (o.ok) {
        const FileRec& rec = tb.recs[o.file];
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
//   counts (may be null)                as file_walk.hip's merge
__global__ __launch_bounds__(256) void files_merge_kernel(FilesTables tb, const uint8_t* __restrict__ path,
    const uint8_t* __restrict__ read, uint64_t e0, uint64_t n, uint8_t* __restrict__ status_out,
    const uint32_t* __restrict__ pointer_in, uint32_t* __restrict__ pointer_out, uint8_t* __restrict__ out, uint64_t out_bytes,
    uint64_t ds, uint32_t* __restrict__ flags, uint32_t flag_shift, unsigned long long* __restrict__ counts, int slot0)
{
    __shared__ uint32_t part[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
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
        if (kOwnerAllLanes || want) {
            const Owner o = owner_of(tb, e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, want);
            if (o.ok) {
                const uint32_t bit = filesplan::flag_of(s) << flag_shift;
                if (flags && bit && PPFS_DBG_OK(flags + o.file, 4, flags, tb.nfiles * 4))
                    atomicOr(flags + o.file, bit);
                if (fill) {
                    const FileRec& rec = tb.recs[o.file];
                    const fileplan::Extent x = fileplan::extent_of(o.k, rec.off0, rec.bytes, ds);
                    const uint64_t at = rec.out_pos + x.pos;
                    for (uint32_t b = 0; b < x.length; ++b)
                        if (x.pos + b < rec.bytes && at + b < out_bytes && PPFS_DBG_OK(out + at + b, 1, out, out_bytes))
                            out[at + b] = 0;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            c[q] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(slot == q));
    }
    if (!counts)
        return;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            part[wave][q] = c[q];
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        const uint32_t q = threadIdx.x;
        const unsigned long long sum = (unsigned long long)part[0][q] + part[1][q] + part[2][q] + part[3][q];
        if (sum && PPFS_DBG_OK(counts + slot0 + q, 8, counts, 64))
            atomicAdd(counts + slot0 + q, sum);
    }
}

// written[f] = file f's bytes, one lane per file: what a batch write reports for a file none of whose blocks
// fails (the write merge lowers it)
__global__ __launch_bounds__(256) void files_written_init_kernel(const FileRec* __restrict__ recs, uint64_t nfiles,
    unsigned long long* __restrict__ written)
{
    const uint64_t f = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (f < nfiles && PPFS_DBG_OK(recs + f, 128, recs, nfiles * 128) && PPFS_DBG_OK(written + f, 8, written, nfiles * 8))
        written[f] = recs[f].bytes;
}

// The merge of a batch WRITE over the merged file blocks e0 + i, i < n: the final status is path[i] where that
// is non-zero, else wst[i], the write's.  It reads and writes no payload byte.
//   status_out (may be null)   the final statuses
//   flags (may be null)        as files_merge_kernel's, the data bits
//   written (may be null)      written[file] lowered to the block's position within its file's bytes for a final
//                              status 5 or 9: a 64-bit atomicMin from the first lane of every run of such lanes of
//                              one file within a wave (positions grow along a file's entries)
//   counts (may be null)       the tally into the file half
__global__ __launch_bounds__(256) void files_write_merge_kernel(FilesTables tb, const uint8_t* __restrict__ path,
    const uint8_t* __restrict__ wst, uint64_t e0, uint64_t n, uint8_t* __restrict__ status_out, uint64_t ds,
    uint32_t* __restrict__ flags, unsigned long long* __restrict__ written, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t part[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
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
        if (kOwnerAllLanes || want)
            o = owner_of(tb, e0 + w0, n - w0 < 256u ? n - w0 : 256u, e0 + i, want);
        const bool stop = o.ok && written && bad;
        const unsigned long long stopped = __builtin_amdgcn_ballot_w64(stop);
        const uint32_t file_before = (uint32_t)__shfl_up((int)o.file, 1);
        const bool continues = lane > 0u && ((stopped >> (lane - 1u)) & 1ull) && file_before == o.file;
        if (o.ok) {
            const uint32_t bit = filesplan::flag_of(s);
            if (flags && bit && PPFS_DBG_OK(flags + o.file, 4, flags, tb.nfiles * 4))
                atomicOr(flags + o.file, bit);
            if (stop && !continues && PPFS_DBG_OK(written + o.file, 8, written, tb.nfiles * 8)) {
                const FileRec& rec = tb.recs[o.file];
                const uint64_t pos = fileplan::extent_of(o.k, rec.off0, rec.bytes, ds).pos;
                atomicMin(written + o.file, (unsigned long long)(pos < rec.bytes ? pos : rec.bytes));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            c[q] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(slot == q));
    }
    if (!counts)
        return;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            part[wave][q] = c[q];
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        const uint32_t q = threadIdx.x;
        const unsigned long long sum = (unsigned long long)part[0][q] + part[1][q] + part[2][q] + part[3][q];
        if (sum && PPFS_DBG_OK(counts + fileplan::SLOT_FILE + q, 8, counts, 64))
            atomicAdd(counts + fileplan::SLOT_FILE + q, sum);
    }
}

static bool grid_of(uint64_t n, uint32_t& grid)
{
    const uint64_t g = (n + 255u) / 256u;
    grid = (uint32_t)g;
    return g <= 0x7FFFFFFFull;
}
static bool tables_ok(const void* recs, uint64_t nfiles, const void* rows, uint64_t nrows)
{
    return recs && rows && nfiles >= 1 && nfiles < 0xFFFFFFFFull && nrows >= 1 && nrows <= nfiles
        && !(((uintptr_t)recs | (uintptr_t)rows) & 7u);
}

} // namespace ppfs

using namespace ppfs;

extern "C" hipError_t ppfs_files_expand_launch(const void* recs, uint64_t nfiles, const void* rows, uint64_t nrows, int level,
    uint64_t e0, uint64_t n, uint64_t ds, const uint8_t* payload, const uint8_t* st, const uint8_t* inh, uint64_t slots,
    uint32_t* pointer, uint8_t* inherited, hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (!tables_ok(recs, nfiles, rows, nrows) || level < fileplan::LEVEL_A || level > fileplan::LEVEL_DATA
        || ((uintptr_t)pointer & 3u) || !grid_of(n, grid))
        return hipErrorInvalidValue;
    const FilesTables tb { (const FileRec*)recs, nfiles, (const Row*)rows, nrows };
    const FilesMem mem { payload, slots * ds, st, inh, slots };
    hipLaunchKernelGGL(files_expand_kernel, dim3(grid), dim3(256), 0, s, tb, mem, level, e0, n, ds, pointer, inherited);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_files_extents_launch(const void* recs, uint64_t nfiles, const void* rows, uint64_t nrows,
    const uint32_t* pointer, const uint8_t* path, uint64_t e0, uint64_t n, uint64_t ds, ppfs_ecc_extent* ext,
    hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (!tables_ok(recs, nfiles, rows, nrows) || !pointer || !path || !ext || ds == 0 || ds > 0xFFFFu || ((uintptr_t)pointer & 3u)
        || ((uintptr_t)ext & 7u) || !grid_of(n, grid))
        return hipErrorInvalidValue;
    const FilesTables tb { (const FileRec*)recs, nfiles, (const Row*)rows, nrows };
    hipLaunchKernelGGL(files_extents_kernel, dim3(grid), dim3(256), 0, s, tb, pointer, path, e0, n, ds, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_files_merge_launch(const void* recs, uint64_t nfiles, const void* rows, uint64_t nrows,
    const uint8_t* path, const uint8_t* read, uint64_t e0, uint64_t n, uint8_t* status_out, const uint32_t* pointer_in,
    uint32_t* pointer_out, uint8_t* out, uint64_t out_bytes, uint64_t ds, uint32_t* flags, uint32_t flag_shift,
    unsigned long long* counts, int slot0, hipStream_t s)
{
    if (n == 0 || (!status_out && !pointer_out && !out && !counts && !flags))
        return hipSuccess;
    if (!tables_ok(recs, nfiles, rows, nrows) || !path || (pointer_out && !pointer_in)
        || (((uintptr_t)pointer_in | (uintptr_t)pointer_out | (uintptr_t)flags) & 3u) || ((uintptr_t)counts & 7u)
        || (slot0 != fileplan::SLOT_FILE && slot0 != fileplan::SLOT_INDEX) || flag_shift > 8u || (out && ds == 0))
        return hipErrorInvalidValue;
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(want < 2048u ? want : 2048u);
    const FilesTables tb { (const FileRec*)recs, nfiles, (const Row*)rows, nrows };
    hipLaunchKernelGGL(files_merge_kernel, dim3(grid), dim3(256), 0, s, tb, path, read, e0, n, status_out,
            pointer_out ? pointer_in : nullptr, pointer_out, out, out_bytes, ds, flags, flag_shift, counts, slot0);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_files_written_init_launch(const void* recs, uint64_t nfiles, unsigned long long* written, hipStream_t s)
{
    uint32_t grid;
    if (!written || nfiles == 0)
        return hipSuccess;
    if (!recs || nfiles >= 0xFFFFFFFFull || (((uintptr_t)recs | (uintptr_t)written) & 7u) || !grid_of(nfiles, grid))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(files_written_init_kernel, dim3(grid), dim3(256), 0, s, (const FileRec*)recs, nfiles, written);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_files_write_merge_launch(const void* recs, uint64_t nfiles, const void* rows, uint64_t nrows,
    const uint8_t* path, const uint8_t* wst, uint64_t e0, uint64_t n, uint8_t* status_out, uint64_t ds, uint32_t* flags,
    unsigned long long* written, unsigned long long* counts, hipStream_t s)
{
    if (n == 0 || (!status_out && !flags && !written && !counts))
        return hipSuccess;
    if (!tables_ok(recs, nfiles, rows, nrows) || !path || ((uintptr_t)flags & 3u) || (((uintptr_t)written | (uintptr_t)counts) & 7u)
        || ds == 0)
        return hipErrorInvalidValue;
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(want < 2048u ? want : 2048u);
    const FilesTables tb { (const FileRec*)recs, nfiles, (const Row*)rows, nrows };
    hipLaunchKernelGGL(files_write_merge_kernel, dim3(grid), dim3(256), 0, s, tb, path, wst, e0, n, status_out, ds, flags, written,
        counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_files_faults)
