// inode_walk.hip -- the kernels of the inode reads (inode_path.cpp; include/ppfs_ecc.h ppfs_ecc_read_inodes_*) and,
// in the second half, of the inode writes (ppfs_ecc_write_inodes_*).
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
#include "inode_wplan.hpp"
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

// ---- the inode writes (inode_path.cpp ppfs_ecc_write_inodes_device; the grouping step of inode_wplan.hpp) ----
//   inode_elect_kernel          one lane per slot (entry j, piece k): a slot that takes part claims its block's key and
//                               lowers the block's owner to its slot index; piece 0 claims the inode number's key and
//                               raises its winner to j
//   inode_owner_extents_kernel  the owner slot of each block emits {pos 0, block, 0, 0}, every other slot the invalid
//                               extent
//   inode_overlay_kernel        inside the extent write, after the old payloads: the slots of winning entries store
//                               their bytes of the composed row into their block's owner row of P
//   inode_write_status_kernel   one lane per inode: the pieces' write statuses under the first toucher rule, the status
//                               rule, status, piece_status, the tally
// The tables were cleared to 0xFF on the stream before the elect kernel.  No lane waits for another: claim() and
// find() end after at most cap probes.
using namespace inodewplan;

// the memory operations of inode_wplan.hpp on the device: a[i], i < cap
struct DeviceOps {
    __device__ static uint32_t load(const uint32_t* a, uint32_t i, uint32_t cap)
    {
        return i < cap && PPFS_DBG_OK(a + i, 4, a, (uint64_t)cap * 4) ? a[i] : EMPTY;
    }
    __device__ static uint32_t cas(uint32_t* a, uint32_t i, uint32_t cap, uint32_t expect, uint32_t v)
    {
        return i < cap && PPFS_DBG_OK(a + i, 4, a, (uint64_t)cap * 4) ? atomicCAS(a + i, expect, v) : 0u;
    }
    __device__ static void min_u32(uint32_t* a, uint32_t i, uint32_t cap, uint32_t v)
    {
        if (i < cap && PPFS_DBG_OK(a + i, 4, a, (uint64_t)cap * 4))
            atomicMin(a + i, v);
    }
    __device__ static void max_i32(uint32_t* a, uint32_t i, uint32_t cap, uint32_t v)
    {
        if (i < cap && PPFS_DBG_OK(a + i, 4, a, (uint64_t)cap * 4))
            atomicMax((int*)(a + i), (int)v);
    }
};

// what slot `slot` < n * K of the piece does, from the scratch; *ino_out and *entry: its inode number and entry
__device__ inline Slot slot_from_scratch(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, uint64_t n, const InodeTable& t, uint64_t ds, uint32_t K, uint64_t slot, uint32_t* ino_out,
    uint32_t* entry)
{
    const uint64_t j = slot / K;
    *entry = (uint32_t)j;
    *ino_out = 0;
    if (j >= n || !PPFS_DBG_OK(ino_in + j, 4, ino_in, n * 4))
        return Slot { false, NO_BLOCK, 0, 0, 0 };
    const uint32_t ino = ino_in[j];
    *ino_out = ino;
    uint32_t bitmap_status;
    const uint32_t verdict = verdict_of(t, ino, bm, bst, j, n, 0x80u >> (ino % 8u), &bitmap_status);
    return slot_of(t.table_block, ino, (uint32_t)(slot - j * K), verdict, ds);
}

// tab: the two tables, table_bytes(cap) bytes, cleared
__global__ __launch_bounds__(256) void inode_elect_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, uint64_t n, InodeTable t, uint64_t ds, uint32_t K, uint32_t* tab, uint32_t cap)
{
    const Tables T = tables_at(tab, cap);
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n * K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(ino_in, bm, bst, n, t, ds, K, s, &ino, &j);
        elect<DeviceOps>(T, sl, ino, j, (uint32_t)(s - (uint64_t)j * K), (uint32_t)s);
    }
}

// ext[s] for s < n * K
__global__ __launch_bounds__(256) void inode_owner_extents_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, uint64_t n, InodeTable t, uint64_t ds, uint32_t K, uint32_t* tab, uint32_t cap,
    ppfs_ecc_extent* __restrict__ ext)
{
    const Tables T = tables_at(tab, cap);
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n * K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(ino_in, bm, bst, n, t, ds, K, s, &ino, &j);
        ppfs_ecc_extent e;
        invalid_extent(e);
        if (sl.takes_part && owner_of<DeviceOps>(T, sl.block) == (uint32_t)s)
            e.block = sl.block; // pos, offset and length 0: the block is checked and encoded again
        if (PPFS_DBG_OK(ext + s, 16, ext, n * K * 16))
            ext[s] = e;
    }
}

// files: 64 n bytes, meta: 3 n 64-bit words; idx[r], r < n * K: the staged index of extent r, whose payload is row r
// of P (stride ds, P_cap bytes)
__global__ __launch_bounds__(256) void inode_overlay_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, uint64_t n, InodeTable t, uint64_t ds, uint32_t K, uint32_t* tab, uint32_t cap,
    const uint8_t* __restrict__ files, const unsigned long long* __restrict__ meta, const uint32_t* __restrict__ idx, uint8_t* P,
    uint64_t P_cap)
{
    const Tables T = tables_at(tab, cap);
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n * K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(ino_in, bm, bst, n, t, ds, K, s, &ino, &j);
        if (!sl.takes_part || winner_of<DeviceOps>(T, ino) != j)
            continue;
        const uint32_t row = owner_of<DeviceOps>(T, sl.block);
        if (row >= n * K || !PPFS_DBG_OK(idx + row, 4, idx, n * K * 4) || idx[row] != sl.block)
            continue; // the block is not in the image: nothing is written
        const uint64_t at = (uint64_t)row * ds + sl.offset;
        if (sl.offset + (uint64_t)sl.length > ds || at + sl.length > P_cap || sl.pos + sl.length > INODE_BYTES
            || !PPFS_DBG_OK(P + at, sl.length, P, P_cap) || !PPFS_DBG_OK(meta + 3ull * j, 24, meta, n * 24)
            || !PPFS_DBG_OK(files + 64ull * j, 64, files, n * 64))
            continue;
        const uint64_t tc = meta[3ull * j], tm = meta[3ull * j + 1u];
        const uint32_t type = (uint32_t)meta[3ull * j + 2u] & 0xFFu;
        const uint8_t* f = files + 64ull * j;
        for (uint32_t b = 0; b < sl.length; ++b)
            P[at + b] = (uint8_t)row_byte(tc, tm, type, [&](uint32_t i) -> uint32_t { return f[i]; }, sl.pos + b);
    }
}

// wst[r], r < n * K: the write status of extent r.  status, piece_status (n * (1 + K) bytes), counts: each may be null
__global__ __launch_bounds__(256) void inode_write_status_kernel(const uint32_t* __restrict__ ino_in, const uint8_t* __restrict__ bm,
    const uint8_t* __restrict__ bst, const uint8_t* __restrict__ wst, uint64_t n, InodeTable t, uint64_t ds, uint32_t K, uint32_t* tab,
    uint32_t cap, uint8_t* __restrict__ status, uint8_t* __restrict__ piece_status, unsigned long long* __restrict__ counts)
{
    const Tables T = tables_at(tab, cap);
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
            auto piece_st = [&](uint32_t k) -> uint32_t {
                const Slot sl = slot_of(t.table_block, ino, k, verdict, ds);
                if (!sl.takes_part)
                    return ST_OUT;
                const uint32_t row = owner_of<DeviceOps>(T, sl.block);
                if (row >= n * K || !PPFS_DBG_OK(wst + row, 1, wst, n * K))
                    return ST_OUT;
                return seen_status(wst[row], (uint32_t)(j * K + k), row);
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

// the inode writes: n inodes of K slots each, n * K <= 2 * PIECE_INODES; tab: 4-byte aligned, table_bytes(cap) bytes
static bool wshape_ok(uint64_t n, uint64_t ds, const void* tab, uint32_t cap)
{
    return shape_ok(n, ds) && n * max_pieces(ds) <= 2u * PIECE_INODES && tab && !((uintptr_t)tab & 3u) && cap >= 2u
        && (cap & (cap - 1u)) == 0u && (uint64_t)cap >= 2u * n * max_pieces(ds);
}

extern "C" hipError_t ppfs_inode_elect_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, ppfs_ecc_extent* ext, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (!ino || !bm || !bst || !table || !ext || ((uintptr_t)ino & 3u) || ((uintptr_t)ext & 7u) || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    const uint32_t K = max_pieces(ds);
    hipLaunchKernelGGL(inode_elect_kernel, dim3(grid_of(n * K)), dim3(256), 0, s, ino, bm, bst, n, t, ds, K, tab, cap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(inode_owner_extents_kernel, dim3(grid_of(n * K)), dim3(256), 0, s, ino, bm, bst, n, t, ds, K, tab, cap, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_overlay_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, const ppfs_ecc_file* files,
    const ppfs_ecc_inode_meta* meta, const uint32_t* idx, uint8_t* P, uint64_t P_cap, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (!ino || !bm || !bst || !table || !files || !meta || !idx || !P || ((uintptr_t)ino & 3u) || ((uintptr_t)idx & 3u)
        || ((uintptr_t)meta & 7u) || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    const uint32_t K = max_pieces(ds);
    hipLaunchKernelGGL(inode_overlay_kernel, dim3(grid_of(n * K)), dim3(256), 0, s, ino, bm, bst, n, t, ds, K, tab, cap,
        (const uint8_t*)files, (const unsigned long long*)meta, idx, P, P_cap);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_write_status_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* wst,
    uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, uint8_t* status, uint8_t* piece_status,
    unsigned long long* counts, hipStream_t s)
{
    if (n == 0 || (!status && !piece_status && !counts))
        return hipSuccess;
    if (!ino || !bm || !bst || !wst || !table || ((uintptr_t)ino & 3u) || ((uintptr_t)counts & 7u) || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    const InodeTable t { table->table_block, table->bitmap_block, table->total_inodes, table->check_bitmap };
    hipLaunchKernelGGL(inode_write_status_kernel, dim3(grid_of(n)), dim3(256), 0, s, ino, bm, bst, wst, n, t, ds, max_pieces(ds), tab,
        cap, status, piece_status, counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_inode_faults)
