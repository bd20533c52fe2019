// inode_walk.hip -- the kernels of the inode reads (inode_path.cpp; include/ppfs_ecc.h ppfs_ecc_read_inodes_*).
//
// InodeManager::get (lib/inode_manager/src/inode_manager.cpp:127-138) is one byte of the inode bitmap, then the 81
// bytes of the packed Inode out of the inode table, cut at block boundaries.  For a piece of a batch of inode
// numbers that is two extent reads with three small kernels around them, all queued, nothing read back:
//   inode_bitmap_extents_kernel  the lane's inode number out of the caller's strided source (byte loads when the
//                                source is not 4-aligned) into the scratch; the extent of its bitmap byte, invalid
//                                when the number is out of range or the bitmap is not checked
//   inode_table_extents_kernel   the bit and its read status decide (inode_plan.hpp bitmap_verdict); K extents,
//                                those of the inode's pieces valid when the table is read, pos = 81 j + the bytes
//                                before piece k
//   inode_merge_kernel           the status rule (inode_plan.hpp), the 81-byte row split into the ppfs_ecc_file
//                                record and the metadata or both zero-filled, status, piece_status, the tally
// One lane per inode, 256 lanes a workgroup, a grid-stride loop; consecutive lanes store consecutive elements.
// The kernels are latency-bound and small: the codec work is in the extent calls between them.  Every index is
// checked against its array's extent before use; all arithmetic is inode_plan.hpp's.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "inode_plan.hpp"
#include "kernels.hpp"
#include "status_tally.hpp"
#include <stdint.h>

namespace ppfs {

using namespace inodeplan;

struct InodeTable {
    uint32_t table_block, bitmap_block, total_inodes, check_bitmap;
};

__device__ inline void invalid_extent(ppfs_ecc_extent& e)
{
    e.pos = 0;
    e.block = NO_BLOCK;
    e.offset = e.length = 0;
}

// src: n numbers `stride` bytes apart, src_bytes = (n - 1) * stride + 4 in all; ino_out[j] and ext[j] for j < n
__global__ __launch_bounds__(256) void inode_bitmap_extents_kernel(const uint8_t* __restrict__ src, uint64_t stride,
    uint64_t src_bytes, uint64_t n, InodeTable t, uint64_t ds, uint32_t* __restrict__ ino_out, ppfs_ecc_extent* __restrict__ ext)
{
    const bool aligned = ((((uintptr_t)src) | stride) & 3u) == 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
        const uint64_t at = j * stride;
        if (at + 4u > src_bytes || !PPFS_DBG_OK(src + at, 4, src, src_bytes))
            continue;
        uint32_t ino;
        if (aligned)
            ino = *(const uint32_t*)(src + at);
        else
            ino = (uint32_t)src[at] | (uint32_t)src[at + 1u] << 8 | (uint32_t)src[at + 2u] << 16 | (uint32_t)src[at + 3u] << 24;
        ppfs_ecc_extent e;
        invalid_extent(e);
        if (ino < t.total_inodes && t.check_bitmap) {
            const BitByte b = bitmap_byte(t.bitmap_block, ino, ds);
            if (b.block < NO_BLOCK) {
                e.pos = j;
                e.block = (uint32_t)b.block;
                e.offset = (uint16_t)b.offset;
                e.length = 1;
            }
        }
        if (PPFS_DBG_OK(ino_out + j, 4, ino_out, n * 4))
            ino_out[j] = ino;
        if (PPFS_DBG_OK(ext + j, 16, ext, n * 16))
            ext[j] = e;
    }
}

// what steps 1 and 2 decide for inode j of the piece, from the scratch
__device__ inline uint32_t verdict_of(const InodeTable& t, uint32_t ino, const uint8_t* __restrict__ bm, const uint8_t* __restrict__ bst,
    uint64_t j, uint64_t n, uint32_t mask, uint32_t* read_status)
{
    uint32_t st = ST_OUT, byte = 0;
    if (ino < t.total_inodes && t.check_bitmap && PPFS_DBG_OK(bst + j, 1, bst, n) && PPFS_DBG_OK(bm + j, 1, bm, n)) {
        st = bst[j];
        if (st == ST_OK || st == ST_CORRECTED) // a byte that was not delivered is not looked at
            byte = bm[j];
    }
    *read_status = st;
    return bitmap_verdict(ino, t.total_inodes, t.check_bitmap != 0, st, byte, mask);
}

// ext[j * K + k], k < K, for j < n
__global__ __launch_bounds__(256) void inode_table_extents_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, uint64_t n, InodeTable t, uint64_t ds, uint32_t K, ppfs_ecc_extent* __restrict__ ext)
{
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u) {
        if (!PPFS_DBG_OK(ino_in + j, 4, ino_in, n * 4))
            continue;
        const uint32_t ino = ino_in[j];
        uint32_t bitmap_status;
        const uint32_t verdict = verdict_of(t, ino, bm, bst, j, n, 0x80u >> (ino % 8u), &bitmap_status);
        const uint32_t np = verdict == 0u ? pieces(ino, ds) : 0u;
        for (uint32_t k = 0; k < K; ++k) {
            ppfs_ecc_extent e;
            invalid_extent(e);
            if (k < np) {
                const Piece p = piece(t.table_block, ino, k, ds);
                if (p.block < NO_BLOCK) {
                    e.pos = (uint64_t)INODE_BYTES * j + p.pos;
                    e.block = (uint32_t)p.block;
                    e.offset = (uint16_t)p.offset;
                    e.length = (uint16_t)p.length;
                }
            }
            if (PPFS_DBG_OK(ext + j * K + k, 16, ext, n * K * 16))
                ext[j * K + k] = e;
        }
    }
}

// rows: 81 n bytes, row j at 81 j (any alignment); pst[j * K + k]: the read status of piece k of inode j.
// files (4-byte aligned), meta (8-byte aligned), status, piece_status (n * (1 + K) bytes), counts: each may be null
__global__ __launch_bounds__(256) void inode_merge_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, const uint8_t* __restrict__ rows, const uint8_t* __restrict__ pst, uint64_t n, InodeTable t,
    uint64_t ds, uint32_t K, uint32_t* __restrict__ files, unsigned long long* __restrict__ meta, uint8_t* __restrict__ status,
    uint8_t* __restrict__ piece_status, unsigned long long* __restrict__ counts)
{
    uint32_t c[4] = { 0, 0, 0, 0 }, free_c[4] = { 0, 0, 0, 0 };
    const uint64_t W = 1u + K;
    for (uint64_t w0 = (uint64_t)blockIdx.x * 256u; w0 < n; w0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t j = w0 + threadIdx.x;
        int slot = -1;
        if (j < n && PPFS_DBG_OK(ino_in + j, 4, ino_in, n * 4)) {
            const uint32_t ino = ino_in[j];
            uint32_t bitmap_status;
            const uint32_t verdict = verdict_of(t, ino, bm, bst, j, n, 0x80u >> (ino % 8u), &bitmap_status);
            const bool bit_read = ino < t.total_inodes && t.check_bitmap;
            const uint32_t np = verdict == 0u ? pieces(ino, ds) : 0u;
            const uint8_t* my = pst + j * K;
            auto piece_st = [&](uint32_t k) -> uint32_t {
                return k < K && PPFS_DBG_OK(my + k, 1, pst, n * K) ? my[k] : (uint32_t)ST_OUT;
            };
            const uint32_t st = verdict ? verdict : table_status(bit_read ? bitmap_status : 0u, np, piece_st);
            slot = count_slot(st);
            if (status && PPFS_DBG_OK(status + j, 1, status, n))
                status[j] = (uint8_t)st;
            if (piece_status) {
                uint8_t* ps = piece_status + j * W;
                if (PPFS_DBG_OK(ps, W, piece_status, n * W)) {
                    ps[0] = (uint8_t)(bit_read ? bitmap_status : ST_UNUSED);
                    for (uint32_t k = 0; k < K; ++k)
                        ps[1u + k] = (uint8_t)(k < np ? piece_st(k) : ST_UNUSED);
                }
            }
            const bool good = st == ST_OK || st == ST_CORRECTED;
            const uint8_t* row = rows + (uint64_t)INODE_BYTES * j;
            auto at = [&](uint32_t i) -> uint32_t {
                return good && i < INODE_BYTES && PPFS_DBG_OK(row + i, 1, rows, (uint64_t)INODE_BYTES * n) ? row[i] : 0u;
            };
            if (files && PPFS_DBG_OK(files + j * 16u, 64, files, n * 64)) {
                for (uint32_t w = 0; w < FILE_BYTES / 4u; ++w)
                    files[j * 16u + w] = le32(at, FILE_OFF + 4u * w);
            }
            if (meta && PPFS_DBG_OK(meta + j * 3u, 24, meta, n * 24)) {
                meta[j * 3u] = le64(at, 0);
                meta[j * 3u + 1u] = le64(at, 8);
                meta[j * 3u + 2u] = at(TYPE_OFF);
            }
        }
        tally_add(c, slot);
        tally_add(free_c, slot == SLOT_NOT_ALLOCATED ? 0 : -1);
    }
    tally_flush(c, counts, 0, 4);
    __syncthreads(); // the two flushes share their LDS words
    tally_flush(free_c, counts, SLOT_NOT_ALLOCATED, 1);
}

// grid-stride, at most 2,048 workgroups
static uint32_t grid_of(uint64_t n)
{
    const uint64_t want = (n + 255u) / 256u;
    return (uint32_t)(want < 2048u ? want : 2048u);
}
static bool shape_ok(uint64_t n, uint64_t ds) { return ds > 0 && ds <= 0xFFFFu && n <= 2u * PIECE_INODES; }

} // namespace ppfs

using namespace ppfs;

extern "C" hipError_t ppfs_inode_bitmap_extents_launch(const void* src, uint64_t stride, uint64_t n, const ppfs_ecc_inode_table* table,
    uint64_t ds, uint32_t* ino_out, ppfs_ecc_extent* ext, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (!src || stride < 4 || !table || !ino_out || !ext || ((uintptr_t)ino_out & 3u) || ((uintptr_t)ext & 7u) || !shape_ok(n, ds))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    hipLaunchKernelGGL(inode_bitmap_extents_kernel, dim3(grid_of(n)), dim3(256), 0, s, (const uint8_t*)src, stride, (n - 1) * stride + 4u,
        n, t, ds, ino_out, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_table_extents_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (!ino || !bm || !bst || !table || !ext || ((uintptr_t)ino & 3u) || ((uintptr_t)ext & 7u) || !shape_ok(n, ds))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    hipLaunchKernelGGL(inode_table_extents_kernel, dim3(grid_of(n)), dim3(256), 0, s, ino, bm, bst, n, t, ds, max_pieces(ds), ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_merge_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* rows,
    const uint8_t* pst, uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta,
    uint8_t* status, uint8_t* piece_status, unsigned long long* counts, hipStream_t s)
{
    if (n == 0 || (!files && !meta && !status && !piece_status && !counts))
        return hipSuccess;
    if (!ino || !bm || !bst || !rows || !pst || !table || ((uintptr_t)ino & 3u) || ((uintptr_t)files & 3u)
        || (((uintptr_t)meta | (uintptr_t)counts) & 7u) || !shape_ok(n, ds))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    hipLaunchKernelGGL(inode_merge_kernel, dim3(grid_of(n)), dim3(256), 0, s, ino, bm, bst, rows, pst, n, t, ds, max_pieces(ds),
        (uint32_t*)files, (unsigned long long*)meta, status, piece_status, counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_inode_faults)
