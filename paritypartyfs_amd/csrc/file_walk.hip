// file_walk.hip -- the kernels of the read-only file walk (file_path.cpp; include/ppfs_ecc.h
// ppfs_ecc_file_blocks_*, ppfs_ecc_read_file_*).
//
// A file's index-block tree is at most three levels deep, and how many index blocks a walk over the file
// blocks [j0, j1) visits at each level follows from the range alone (file_plan.hpp).  So the walk is one
// list decode per level with an expansion in between, all queued, nothing read back:
//   file_expand_kernel   one level (or a piece of the file blocks): entry k takes its pointer from slot s
//                        of its parent's decoded payload in the scratch, or from the inode record
//   file_extents_kernel  a piece of file blocks: the ppfs_ecc_extent entries of the read, closed form
//   file_merge_kernel    path status over read status, zero fill under a failed index block, the counts;
//                        for a level of the tree also its pointers and statuses into the caller's arrays
// and of the file write (ppfs_ecc_write_file_*), which reuses the expansion and the extents:
//   file_written_init_kernel  written = the range's bytes
//   file_write_merge_kernel   path status over write status, the counts, written lowered to the first
//                             failing block's position; no payload byte is read or written
// One lane per output element, 256 lanes a workgroup; consecutive lanes store consecutive elements.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "file_plan.hpp"
#include "kernels.hpp"
#include <stdint.h>

namespace ppfs {

// what fileplan::expand reads: the inode record by value, the tree's scratch (slots entries)
struct FileSrc {
    ppfs_ecc_file file;
    const uint8_t* payload; // slots * ds bytes
    uint64_t payload_bytes;
    const uint8_t* st;  // decode statuses, one per slot
    const uint8_t* inh; // inherited path statuses, one per slot
    uint64_t slots;
    __device__ uint32_t inode(uint32_t dw) const { return dw < 16u ? ((const uint32_t*)&file)[dw] : fileplan::NO_BLOCK; }
    __device__ uint32_t status(uint64_t p) const { return PPFS_DBG_OK(st + p, 1, st, slots) && p < slots ? st[p] : 9u; }
    __device__ uint32_t inherited(uint64_t p) const { return PPFS_DBG_OK(inh + p, 1, inh, slots) && p < slots ? inh[p] : 9u; }
    // a byte, never a dword: ds is rarely a multiple of 4 and the last entry of the last payload ends
    // where the scratch's payload area does
    __device__ uint32_t payload_byte(uint64_t at) const
    {
        return PPFS_DBG_OK(payload + at, 1, payload, payload_bytes) && at < payload_bytes ? payload[at] : 0xFFu;
    }
};

// entries [k0, k0 + n) of a level: pointer[i] and inherited[i] for entry k0 + i (either may be null)
__global__ __launch_bounds__(256) void file_expand_kernel(FileSrc src, fileplan::Tree tree, int level, uint64_t k0, uint64_t n,
    uint64_t ds, uint32_t* __restrict__ pointer, uint8_t* __restrict__ inherited)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const fileplan::Expanded e = fileplan::expand(tree, level, k0 + i, ds, src);
    if (pointer && PPFS_DBG_OK(pointer + i, 4, pointer, n * 4))
        pointer[i] = e.pointer;
    if (inherited && PPFS_DBG_OK(inherited + i, 1, inherited, n))
        inherited[i] = e.inherited;
}

// ext[i] = the read of block i0 + i of a file read (i0 + i counted from the read's first block): the
// resolved block, or NO_BLOCK where the path failed, so that the extent call reads nothing for it
__global__ __launch_bounds__(256) void file_extents_kernel(const uint32_t* __restrict__ pointer, const uint8_t* __restrict__ path,
    uint64_t i0, uint64_t n, uint64_t off0, uint64_t bytes, uint64_t ds, ppfs_ecc_extent* __restrict__ ext)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !PPFS_DBG_OK(pointer + i, 4, pointer, n * 4) || !PPFS_DBG_OK(path + i, 1, path, n))
        return;
    const fileplan::Extent x = fileplan::extent_of(i0 + i, off0, bytes, ds);
    ppfs_ecc_extent e;
    e.pos = x.pos;
    e.block = path[i] ? fileplan::NO_BLOCK : pointer[i];
    e.offset = (uint16_t)x.offset;
    e.length = (uint16_t)x.length;
    if (PPFS_DBG_OK(ext + i, 16, ext, n * 16))
        ext[i] = e;
}

// Entries i < n: the final status is path[i] where that is non-zero, else read[i] (null: 0).
//   status_out (may be null)            the final statuses
//   pointer_in / pointer_out (may be null, together)  a level's pointers into the caller's array
//   out (may be null)                   the packed buffer of a file read of `bytes` bytes: the range of a
//                                       block with path status 5 is zero-filled like a failed read's (a
//                                       block with path status 9 is not written); i0, off0, ds as above
//   counts (may be null)                counts[slot0 + fileplan::count_slot(final)] grows by one
// The tally is alloc_scan.hip's: wave ballots, the four waves through LDS, one 64-bit atomicAdd per
// category and workgroup.  The record was zeroed on the stream before.
__global__ __launch_bounds__(256) void file_merge_kernel(const uint8_t* __restrict__ path, const uint8_t* __restrict__ read,
    uint64_t n, uint8_t* __restrict__ status_out, const uint32_t* __restrict__ pointer_in, uint32_t* __restrict__ pointer_out,
    uint8_t* __restrict__ out, uint64_t i0, uint64_t off0, uint64_t bytes, uint64_t ds, unsigned long long* __restrict__ counts,
    int slot0)
{
    __shared__ uint32_t part[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t c[4] = { 0, 0, 0, 0 };
    for (uint64_t k0 = (uint64_t)blockIdx.x * 256u; k0 < n; k0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = k0 + threadIdx.x;
        int slot = -1;
        if (i < n && PPFS_DBG_OK(path + i, 1, path, n)) {
            const uint32_t p = path[i];
            const uint32_t s = p ? p : (read && PPFS_DBG_OK(read + i, 1, read, n) ? read[i] : 0u);
            slot = fileplan::count_slot(s);
            if (status_out && PPFS_DBG_OK(status_out + i, 1, status_out, n))
                status_out[i] = (uint8_t)s;
            if (pointer_out && PPFS_DBG_OK(pointer_in + i, 4, pointer_in, n * 4) && PPFS_DBG_OK(pointer_out + i, 4, pointer_out, n * 4))
                pointer_out[i] = pointer_in[i];
            if (out && p == fileplan::STATUS_FAILED) {
                const fileplan::Extent x = fileplan::extent_of(i0 + i, off0, bytes, ds);
                for (uint32_t b = 0; b < x.length; ++b)
                    if (x.pos + b < bytes && PPFS_DBG_OK(out + x.pos + b, 1, out, bytes))
                        out[x.pos + b] = 0;
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

// *written = bytes: what a file write reports when no block of its range fails (the write merge lowers it)
__global__ __launch_bounds__(64) void file_written_init_kernel(unsigned long long* __restrict__ written, uint64_t bytes)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && PPFS_DBG_OK(written, 8, written, 8))
        *written = bytes;
}

// The merge of a file WRITE over the blocks i0 + i, i < n, of a range of `bytes` bytes: the final status is
// path[i] where that is non-zero, else wst[i], the write's.  It reads and writes no payload byte.
//   status_out (may be null)   the final statuses
//   written (may be null)      lowered to the pos of the first block whose final status is 5 or 9.  pos grows
//                              with i, so of a wave only its first such lane issues the 64-bit atomicMin
//   counts (may be null)       file_merge_kernel's tally into the file half
__global__ __launch_bounds__(256) void file_write_merge_kernel(const uint8_t* __restrict__ path, const uint8_t* __restrict__ wst,
    uint64_t n, uint8_t* __restrict__ status_out, uint64_t i0, uint64_t off0, uint64_t bytes, uint64_t ds,
    unsigned long long* __restrict__ written, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t part[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t c[4] = { 0, 0, 0, 0 };
    for (uint64_t k0 = (uint64_t)blockIdx.x * 256u; k0 < n; k0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = k0 + threadIdx.x;
        int slot = -1;
        if (i < n && PPFS_DBG_OK(path + i, 1, path, n)) {
            const uint32_t p = path[i];
            const uint32_t s = p ? p : (wst && PPFS_DBG_OK(wst + i, 1, wst, n) ? wst[i] : 0u);
            slot = fileplan::count_slot(s);
            if (status_out && PPFS_DBG_OK(status_out + i, 1, status_out, n))
                status_out[i] = (uint8_t)s;
        }
        const unsigned long long stopped = __builtin_amdgcn_ballot_w64(slot == 2 || slot == 3);
        if (written && stopped && lane == (uint32_t)__builtin_ctzll(stopped) && PPFS_DBG_OK(written, 8, written, 8)) {
            const uint64_t pos = fileplan::extent_of(i0 + i, off0, bytes, ds).pos;
            atomicMin(written, (unsigned long long)(pos < bytes ? pos : bytes));
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

} // namespace ppfs

using namespace ppfs;

extern "C" hipError_t ppfs_file_expand_launch(const ppfs_ecc_file* file, const fileplan::Tree* tree, int level, uint64_t k0,
    uint64_t n, uint64_t ds, const uint8_t* payload, const uint8_t* st, const uint8_t* inh, uint32_t* pointer, uint8_t* inherited,
    hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (!file || !tree || level < fileplan::LEVEL_A || level > fileplan::LEVEL_DATA || k0 + n > fileplan::level_count(*tree, level)
        || ((uintptr_t)pointer & 3u) || !grid_of(n, grid))
        return hipErrorInvalidValue;
    const uint64_t slots = fileplan::tree_slots(*tree);
    const FileSrc src { *file, payload, slots * ds, st, inh, slots };
    hipLaunchKernelGGL(file_expand_kernel, dim3(grid), dim3(256), 0, s, src, *tree, level, k0, n, ds, pointer, inherited);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_file_extents_launch(const uint32_t* pointer, const uint8_t* path, uint64_t i0, uint64_t n, uint64_t off0,
    uint64_t bytes, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s)
{
    uint32_t grid;
    if (n == 0)
        return hipSuccess;
    if (!pointer || !path || !ext || ds == 0 || ds > 0xFFFFu || off0 >= ds || ((uintptr_t)pointer & 3u) || ((uintptr_t)ext & 7u)
        || !grid_of(n, grid))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(file_extents_kernel, dim3(grid), dim3(256), 0, s, pointer, path, i0, n, off0, bytes, ds, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_file_merge_launch(const uint8_t* path, const uint8_t* read, uint64_t n, uint8_t* status_out,
    const uint32_t* pointer_in, uint32_t* pointer_out, uint8_t* out, uint64_t i0, uint64_t off0, uint64_t bytes, uint64_t ds,
    unsigned long long* counts, int slot0, hipStream_t s)
{
    if (n == 0 || (!status_out && !pointer_out && !out && !counts))
        return hipSuccess;
    if (!path || (pointer_out && !pointer_in) || (((uintptr_t)pointer_in | (uintptr_t)pointer_out) & 3u) || ((uintptr_t)counts & 7u)
        || (slot0 != fileplan::SLOT_FILE && slot0 != fileplan::SLOT_INDEX) || (out && (ds == 0 || off0 >= ds)))
        return hipErrorInvalidValue;
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(want < 2048u ? want : 2048u);
    hipLaunchKernelGGL(file_merge_kernel, dim3(grid), dim3(256), 0, s, path, read, n, status_out, pointer_out ? pointer_in : nullptr,
        pointer_out, out, i0, off0, bytes, ds, counts, slot0);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_file_written_init_launch(unsigned long long* written, uint64_t bytes, hipStream_t s)
{
    if (!written)
        return hipSuccess;
    if ((uintptr_t)written & 7u)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(file_written_init_kernel, dim3(1), dim3(64), 0, s, written, bytes);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_file_write_merge_launch(const uint8_t* path, const uint8_t* wst, uint64_t n, uint8_t* status_out,
    uint64_t i0, uint64_t off0, uint64_t bytes, uint64_t ds, unsigned long long* written, unsigned long long* counts, hipStream_t s)
{
    if (n == 0 || (!status_out && !written && !counts))
        return hipSuccess;
    if (!path || (((uintptr_t)written | (uintptr_t)counts) & 7u) || ds == 0 || off0 >= ds)
        return hipErrorInvalidValue;
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(want < 2048u ? want : 2048u);
    hipLaunchKernelGGL(file_write_merge_kernel, dim3(grid), dim3(256), 0, s, path, wst, n, status_out, i0, off0, bytes, ds, written,
        counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_file_faults)
