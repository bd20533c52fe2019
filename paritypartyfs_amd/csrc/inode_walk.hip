// inode_walk.hip -- the kernels of the inode reads (inode_path.cpp; include/ppfs_ecc.h ppfs_ecc_read_inodes_*) and,
// in the second half, of the inode writes (ppfs_ecc_write_inodes_*).
//
// InodeManager::get (lib/inode_manager/src/inode_manager.cpp:127-138) is one byte of the inode bitmap, then the 81
// bytes of the packed Inode out of the inode table, cut at block boundaries.  For a piece of a batch of inode
// numbers that is two extent reads with three small kernels around them, all queued, nothing read back:
//   inode_bitmap_extents_kernel      the lane's inode number out of the caller's strided source (byte loads when the
//                                    source is not 4-aligned) into the scratch; the extent of its bitmap byte, invalid
//                                    when the number is out of range or the bitmap is not checked
//   inode_table_extents_kernel       the bit and its read status decide (inode_plan.hpp bitmap_step); K extents, those
//                                    of the slots that take part valid (slot_of, slot_extent)
//   inode_status_kernel<ReadPieces>  the epilogue (inode_plan.hpp inode_status): status, piece_status, the tally; the
//                                    81-byte row split into the ppfs_ecc_file record and the metadata or both zero-filled
// One lane per inode, 256 lanes a workgroup, a grid-stride loop; consecutive lanes store consecutive elements.
// The kernels are latency-bound and small: the codec work is in the extent calls between them.  Every index is
// checked against its array's extent before use; all arithmetic and the whole per-inode rule are inode_plan.hpp's.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "inode_plan.hpp"
#include "inode_wplan.hpp"
#include "kernels.hpp"
#include "status_tally.hpp"
#include <stdint.h>

namespace ppfs {

using namespace inodeplan;

__device__ inline void invalid_extent(ppfs_ecc_extent& e)
{
    e.pos = 0;
    e.block = NO_BLOCK;
    e.offset = e.length = 0;
}

// src: n numbers `stride` bytes apart, src_bytes = (n - 1) * stride + 4 in all; ino_out[j] and ext[j] for j < n
__global__ __launch_bounds__(256) void inode_bitmap_extents_kernel(const uint8_t* __restrict__ src, uint64_t stride,
    uint64_t src_bytes, uint64_t n, Table t, uint64_t ds, uint32_t* __restrict__ ino_out, ppfs_ecc_extent* __restrict__ ext)
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

// A piece of a batch as the bitmap steps left it in the scratch: ino[j], bm[j], bst[j] for j < n; K = max_pieces(ds).
// What every kernel below starts from.
struct PieceIn {
    const uint32_t* ino;
    const uint8_t *bm, *bst;
    uint64_t n;
    Table t;
    uint64_t ds;
    uint32_t K;
};

// the number of inode j and what steps 1 and 2 decided for it; false when there is no such inode
__device__ inline bool inode_at(const PieceIn& p, uint64_t j, uint32_t* ino, BitmapStep* b)
{
    if (j >= p.n || !PPFS_DBG_OK(p.ino + j, 4, p.ino, p.n * 4))
        return false;
    *ino = p.ino[j];
    uint32_t st = ST_OUT, byte = 0;
    if (PPFS_DBG_OK(p.bst + j, 1, p.bst, p.n) && PPFS_DBG_OK(p.bm + j, 1, p.bm, p.n)) {
        st = p.bst[j];
        byte = p.bm[j];
    }
    *b = bitmap_step(p.t, *ino, byte, st);
    return true;
}

// ext[j * K + k], k < K, for j < n
__global__ __launch_bounds__(256) void inode_table_extents_kernel(PieceIn p, ppfs_ecc_extent* __restrict__ ext)
{
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < p.n; j += (uint64_t)gridDim.x * 256u) {
        uint32_t ino = 0;
        BitmapStep b {};
        if (!inode_at(p, j, &ino, &b))
            continue;
        for (uint32_t k = 0; k < p.K; ++k)
            if (PPFS_DBG_OK(ext + j * p.K + k, 16, ext, p.n * p.K * 16))
                ext[j * p.K + k] = slot_extent<ppfs_ecc_extent>(slot_of(p.t.table_block, ino, k, b.verdict, p.ds), j);
    }
}

// Where the read's piece statuses come from: pst[j * K + k], the read status of piece k of inode j.  Its inodes have
// a row to split: rows, 81 n bytes, row j at 81 j (any alignment), into files (4-byte aligned) and meta (8-byte
// aligned), each may be null
struct ReadPieces {
    const uint8_t *rows, *pst;
    uint32_t* files;
    unsigned long long* meta;

    __device__ uint32_t status(const PieceIn& p, uint64_t j, uint32_t, uint32_t, uint32_t k) const
    {
        const uint8_t* my = pst + j * p.K + k;
        return k < p.K && PPFS_DBG_OK(my, 1, pst, p.n * p.K) ? *my : (uint32_t)ST_OUT;
    }
    __device__ void finish(const PieceIn& p, uint64_t j, uint32_t st) const
    {
        const bool good = st == ST_OK || st == ST_CORRECTED;
        const uint8_t* row = rows + (uint64_t)INODE_BYTES * j;
        auto at = [&](uint32_t i) -> uint32_t {
            return good && i < INODE_BYTES && PPFS_DBG_OK(row + i, 1, rows, (uint64_t)INODE_BYTES * p.n) ? row[i] : 0u;
        };
        if (files && PPFS_DBG_OK(files + j * 16u, 64, files, p.n * 64)) {
            for (uint32_t w = 0; w < FILE_BYTES / 4u; ++w)
                files[j * 16u + w] = le32(at, FILE_OFF + 4u * w);
        }
        if (meta && PPFS_DBG_OK(meta + j * 3u, 24, meta, p.n * 24)) {
            meta[j * 3u] = le64(at, 0);
            meta[j * 3u + 1u] = le64(at, 8);
            meta[j * 3u + 2u] = at(TYPE_OFF);
        }
    }
};

// The epilogue of a piece, for the reads and the writes: Pieces::status(p, j, ino, verdict, k) is the status of piece
// k of inode j, Pieces::finish(p, j, st) what else the call stores for an inode of final status st.
// status, piece_status (n * (1 + K) bytes), counts: each may be null
template <class Pieces>
__global__ __launch_bounds__(256) void inode_status_kernel(PieceIn p, Pieces src, uint8_t* __restrict__ status,
    uint8_t* __restrict__ piece_status, unsigned long long* __restrict__ counts)
{
    uint32_t c[4] = { 0, 0, 0, 0 }, free_c[4] = { 0, 0, 0, 0 };
    const uint64_t W = 1u + p.K;
    for (uint64_t w0 = (uint64_t)blockIdx.x * 256u; w0 < p.n; w0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t j = w0 + threadIdx.x;
        int slot = -1;
        uint32_t ino = 0;
        BitmapStep b {};
        if (inode_at(p, j, &ino, &b)) {
            uint8_t* ps = piece_status ? piece_status + j * W : nullptr;
            if (ps && !PPFS_DBG_OK(ps, W, piece_status, p.n * W))
                ps = nullptr;
            const uint32_t st = inode_status(b, ino, p.ds, p.K, [&](uint32_t k) { return src.status(p, j, ino, b.verdict, k); }, ps);
            slot = count_slot(st);
            if (status && PPFS_DBG_OK(status + j, 1, status, p.n))
                status[j] = (uint8_t)st;
            src.finish(p, j, st);
        }
        tally_add(c, slot);
        tally_add(free_c, slot == SLOT_NOT_ALLOCATED ? 0 : -1);
    }
    tally_flush(c, counts, 0, 4);
    __syncthreads(); // the two flushes share their LDS words
    tally_flush(free_c, counts, SLOT_NOT_ALLOCATED, 1);
}

// ---- the inode writes (inode_path.cpp ppfs_ecc_write_inodes_device; the grouping step of inode_wplan.hpp) ----
//   inode_elect_kernel                one lane per slot (entry j, piece k): a slot that takes part claims its block's
//                                     key and lowers the block's owner to its slot index; piece 0 claims the inode
//                                     number's key and raises its winner to j
//   inode_owner_extents_kernel        the owner slot of each block emits {pos 0, block, 0, 0}, every other slot the
//                                     invalid extent
//   inode_overlay_kernel              inside the extent write, after the old payloads: the slots of winning entries
//                                     store their bytes of the composed row into their block's owner row of P
//   inode_status_kernel<WritePieces>  one lane per inode: the pieces' write statuses under the first toucher rule, then
//                                     the reads' epilogue
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

// what slot `slot` < n * K of the piece does; *ino and *entry: its inode number and entry
__device__ inline Slot slot_from_scratch(const PieceIn& p, uint64_t slot, uint32_t* ino, uint32_t* entry)
{
    const uint64_t j = slot / p.K;
    *entry = (uint32_t)j;
    *ino = 0;
    BitmapStep b {};
    if (!inode_at(p, j, ino, &b))
        return Slot { false, NO_BLOCK, 0, 0, 0 };
    return slot_of(p.t.table_block, *ino, (uint32_t)(slot - j * p.K), b.verdict, p.ds);
}

// T: the two tables, cleared
__global__ __launch_bounds__(256) void inode_elect_kernel(PieceIn p, Tables T)
{
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < p.n * p.K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(p, s, &ino, &j);
        elect<DeviceOps>(T, sl, ino, j, (uint32_t)(s - (uint64_t)j * p.K), (uint32_t)s);
    }
}

// ext[s] for s < n * K
__global__ __launch_bounds__(256) void inode_owner_extents_kernel(PieceIn p, Tables T, ppfs_ecc_extent* __restrict__ ext)
{
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < p.n * p.K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(p, s, &ino, &j);
        ppfs_ecc_extent e;
        invalid_extent(e);
        if (sl.takes_part && owner_of<DeviceOps>(T, sl.block) == (uint32_t)s)
            e.block = sl.block; // pos, offset and length 0: the block is checked and encoded again
        if (PPFS_DBG_OK(ext + s, 16, ext, p.n * p.K * 16))
            ext[s] = e;
    }
}

// files: 64 n bytes, meta: 3 n 64-bit words; idx[r], r < n * K: the staged index of extent r, whose payload is row r
// of P (stride ds, P_cap bytes)
__global__ __launch_bounds__(256) void inode_overlay_kernel(PieceIn p, Tables T, const uint8_t* __restrict__ files,
    const unsigned long long* __restrict__ meta, const uint32_t* __restrict__ idx, uint8_t* P, uint64_t P_cap)
{
    const uint64_t n = p.n, ds = p.ds;
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n * p.K; s += (uint64_t)gridDim.x * 256u) {
        uint32_t ino, j;
        const Slot sl = slot_from_scratch(p, s, &ino, &j);
        if (!sl.takes_part || winner_of<DeviceOps>(T, ino) != j)
            continue;
        const uint32_t row = owner_of<DeviceOps>(T, sl.block);
        if (row >= n * p.K || !PPFS_DBG_OK(idx + row, 4, idx, n * p.K * 4) || idx[row] != sl.block)
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

// Where the write's piece statuses come from: wst[r], r < n * K, the write status of extent r; a piece's is that of
// its block's owner row, found through the tables, under the first toucher rule.  Nothing else to store
struct WritePieces {
    const uint8_t* wst;
    Tables T;

    __device__ uint32_t status(const PieceIn& p, uint64_t j, uint32_t ino, uint32_t verdict, uint32_t k) const
    {
        const Slot sl = slot_of(p.t.table_block, ino, k, verdict, p.ds);
        if (!sl.takes_part)
            return ST_OUT;
        const uint32_t row = owner_of<DeviceOps>(T, sl.block);
        if (row >= p.n * p.K || !PPFS_DBG_OK(wst + row, 1, wst, p.n * p.K))
            return ST_OUT;
        return seen_status(wst[row], (uint32_t)(j * p.K + k), row);
    }
    __device__ void finish(const PieceIn&, uint64_t, uint32_t) const { }
};

// grid-stride, at most 2,048 workgroups
static uint32_t grid_of(uint64_t n)
{
    const uint64_t want = (n + 255u) / 256u;
    return (uint32_t)(want < 2048u ? want : 2048u);
}
static bool shape_ok(uint64_t n, uint64_t ds) { return ds > 0 && ds <= 0xFFFFu && n <= 2u * PIECE_INODES; }
static Table table_of(const ppfs_ecc_inode_table& t) { return Table { t.table_block, t.bitmap_block, t.total_inodes, t.check_bitmap }; }

// what every launcher behind the bitmap step checks of the scratch and the table, and the piece the kernels take
static bool piece_in(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n, const ppfs_ecc_inode_table* table,
    uint64_t ds, PieceIn* p)
{
    if (!ino || !bm || !bst || !table || ((uintptr_t)ino & 3u) || !shape_ok(n, ds))
        return false;
    *p = PieceIn { ino, bm, bst, n, table_of(*table), ds, max_pieces(ds) };
    return true;
}
// the inode writes: n inodes of K slots each, n * K <= 2 * PIECE_INODES; tab: 4-byte aligned, table_bytes(cap) bytes
static bool wshape_ok(uint64_t n, uint64_t ds, const void* tab, uint32_t cap)
{
    return n * max_pieces(ds) <= 2u * PIECE_INODES && tab && !((uintptr_t)tab & 3u) && cap >= 2u && (cap & (cap - 1u)) == 0u
        && (uint64_t)cap >= 2u * n * max_pieces(ds);
}

} // namespace ppfs

using namespace ppfs;

extern "C" hipError_t ppfs_inode_bitmap_extents_launch(const void* src, uint64_t stride, uint64_t n, const ppfs_ecc_inode_table* table,
    uint64_t ds, uint32_t* ino_out, ppfs_ecc_extent* ext, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (!src || stride < 4 || !table || !ino_out || !ext || ((uintptr_t)ino_out & 3u) || ((uintptr_t)ext & 7u) || !shape_ok(n, ds))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_bitmap_extents_kernel, dim3(grid_of(n)), dim3(256), 0, s, (const uint8_t*)src, stride, (n - 1) * stride + 4u,
        n, table_of(*table), ds, ino_out, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_table_extents_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_extent* ext, hipStream_t s)
{
    PieceIn p;
    if (n == 0)
        return hipSuccess;
    if (!piece_in(ino, bm, bst, n, table, ds, &p) || !ext || ((uintptr_t)ext & 7u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_table_extents_kernel, dim3(grid_of(n)), dim3(256), 0, s, p, ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_merge_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* rows,
    const uint8_t* pst, uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta,
    uint8_t* status, uint8_t* piece_status, unsigned long long* counts, hipStream_t s)
{
    PieceIn p;
    if (n == 0 || (!files && !meta && !status && !piece_status && !counts))
        return hipSuccess;
    if (!piece_in(ino, bm, bst, n, table, ds, &p) || !rows || !pst || ((uintptr_t)files & 3u)
        || (((uintptr_t)meta | (uintptr_t)counts) & 7u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_status_kernel<ReadPieces>, dim3(grid_of(n)), dim3(256), 0, s, p,
        ReadPieces { rows, pst, (uint32_t*)files, (unsigned long long*)meta }, status, piece_status, counts);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_elect_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, ppfs_ecc_extent* ext, hipStream_t s)
{
    PieceIn p;
    if (n == 0)
        return hipSuccess;
    if (!piece_in(ino, bm, bst, n, table, ds, &p) || !ext || ((uintptr_t)ext & 7u) || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_elect_kernel, dim3(grid_of(n * p.K)), dim3(256), 0, s, p, tables_at(tab, cap));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(inode_owner_extents_kernel, dim3(grid_of(n * p.K)), dim3(256), 0, s, p, tables_at(tab, cap), ext);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_overlay_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, uint64_t n,
    const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, const ppfs_ecc_file* files,
    const ppfs_ecc_inode_meta* meta, const uint32_t* idx, uint8_t* P, uint64_t P_cap, hipStream_t s)
{
    PieceIn p;
    if (n == 0)
        return hipSuccess;
    if (!piece_in(ino, bm, bst, n, table, ds, &p) || !files || !meta || !idx || !P || ((uintptr_t)idx & 3u) || ((uintptr_t)meta & 7u)
        || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_overlay_kernel, dim3(grid_of(n * p.K)), dim3(256), 0, s, p, tables_at(tab, cap), (const uint8_t*)files,
        (const unsigned long long*)meta, idx, P, P_cap);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_inode_write_status_launch(const uint32_t* ino, const uint8_t* bm, const uint8_t* bst, const uint8_t* wst,
    uint64_t n, const ppfs_ecc_inode_table* table, uint64_t ds, uint32_t* tab, uint32_t cap, uint8_t* status, uint8_t* piece_status,
    unsigned long long* counts, hipStream_t s)
{
    PieceIn p;
    if (n == 0 || (!status && !piece_status && !counts))
        return hipSuccess;
    if (!piece_in(ino, bm, bst, n, table, ds, &p) || !wst || ((uintptr_t)counts & 7u) || !wshape_ok(n, ds, tab, cap))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inode_status_kernel<WritePieces>, dim3(grid_of(n)), dim3(256), 0, s, p, WritePieces { wst, tables_at(tab, cap) },
        status, piece_status, counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_inode_faults)
