// alloc_scan.hip -- the kernels of the allocated-block and block-list scrub (scrub_path.cpp;
// include/ppfs_ecc.h ppfs_ecc_scrub_allocated_*, ppfs_ecc_scrub_list_*).
//
// An allocation bitmap (lib/bitmap/src/bitmap.cpp), decoded into its payload stream, becomes the
// ascending list of the blocks whose bit is set; the list decode then does the codec work over exactly
// those rows, and a tally turns its list-order statuses into per-bit statuses and counts.  The
// arithmetic (bit order, masks, the cut into pieces and chunks) is alloc_plan.hpp, shared with the host
// form and tests/cpp/test_alloc_plan.cpp.
//
// The expansion is a two-pass scan, so that no workgroup ever waits on another:
//   alloc_count_kernel    one workgroup per chunk of 256 words (8,192 bits): the chunk's popcount
//   alloc_offsets_kernel  one workgroup: exclusive scan of a piece's <= 128 chunk totals, and the piece's
//                         total as the 8-byte count the host reads to size the list call
//   alloc_expand_kernel   the same chunks: a lane's offset is its chunk's offset plus the exclusive
//                         prefix of the lanes' popcounts (shuffles within a wave, LDS across the four);
//                         the lane then writes first_block + j for its word's set bits, lowest first
// Both passes form a word the same way (alloc::word_bits), so they agree on every count.
#include <hip/hip_runtime.h>

#include "alloc_plan.hpp"
#include "dbg.hpp"
#include "status_tally.hpp"
#include <stdint.h>

namespace ppfs {

// what alloc::word_bits reads: the bitmap's payload stream (4-byte aligned, stream_bytes = B * ds) and
// the bitmap blocks' statuses
struct AllocSrc {
    const uint8_t* stream;
    uint64_t stream_bytes;
    const uint8_t* bstatus;
    uint64_t B;
    __device__ uint32_t dword(uint64_t w) const
    {
        const uint8_t* p = stream + 4u * w;
        return PPFS_DBG_OK(p, 4, stream, stream_bytes) ? *(const uint32_t*)p : 0u;
    }
    __device__ uint32_t byte(uint64_t i) const { return PPFS_DBG_OK(stream + i, 1, stream, stream_bytes) ? stream[i] : 0u; }
    __device__ uint32_t status(uint64_t b) const { return PPFS_DBG_OK(bstatus + b, 1, bstatus, B) ? bstatus[b] : 0u; }
};

// Exclusive prefix of v over the 256 lanes of a workgroup, and their total: an inclusive scan by
// shuffles within each wave, the four wave totals through LDS.  One call per kernel (wave_tot is not
// guarded against reuse).
__device__ inline uint32_t block_excl_prefix(uint32_t v, uint32_t* wave_tot, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d)
            inc += t;
    }
    if (lane == 63u)
        wave_tot[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t t = wave_tot[k];
        base += k < wave ? t : 0u;
        total += t;
    }
    return base + inc - v;
}

__global__ __launch_bounds__(256) void alloc_count_kernel(AllocSrc src, uint64_t nbits, uint64_t ds, uint64_t word0,
    uint32_t* __restrict__ chunk_tot, uint32_t chunks)
{
    __shared__ uint32_t wave_tot[4];
    const uint64_t w = word0 + (uint64_t)blockIdx.x * alloc::CHUNK_WORDS + threadIdx.x;
    uint32_t total;
    (void)block_excl_prefix((uint32_t)__builtin_popcount(alloc::word_bits(src, w, nbits, ds, src.B)), wave_tot, total);
    if (threadIdx.x == 0 && PPFS_DBG_OK(chunk_tot + blockIdx.x, 4, chunk_tot, (uint64_t)chunks * 4))
        chunk_tot[blockIdx.x] = total;
}

// chunk_off[i] = chunk_tot[0] + .. + chunk_tot[i - 1]; *piece_total = the piece's set bits; the counts
// record's not_allocated grows by the piece's clear bits
__global__ __launch_bounds__(256) void alloc_offsets_kernel(const uint32_t* __restrict__ chunk_tot, uint32_t chunks,
    uint32_t* __restrict__ chunk_off, unsigned long long* __restrict__ piece_total, uint64_t piece_bits,
    unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t wave_tot[4];
    const uint32_t i = threadIdx.x;
    const bool mine = i < chunks;
    const uint32_t v = mine && PPFS_DBG_OK(chunk_tot + i, 4, chunk_tot, (uint64_t)chunks * 4) ? chunk_tot[i] : 0u;
    uint32_t total;
    const uint32_t off = block_excl_prefix(v, wave_tot, total);
    if (mine && PPFS_DBG_OK(chunk_off + i, 4, chunk_off, (uint64_t)chunks * 4))
        chunk_off[i] = off;
    if (i == 0) {
        if (PPFS_DBG_OK(piece_total, 8, piece_total, 8))
            *piece_total = total;
        if (counts && PPFS_DBG_OK(counts + alloc::SLOT_NOT_ALLOCATED, 8, counts, 64))
            atomicAdd(counts + alloc::SLOT_NOT_ALLOCATED, (unsigned long long)(piece_bits - total));
    }
}

// index[chunk_off[chunk] + ...] = first_block + j for the set bits j of the chunk, ascending; cap: the
// entries index holds (the piece's bits)
__global__ __launch_bounds__(256) void alloc_expand_kernel(AllocSrc src, uint64_t nbits, uint64_t ds, uint64_t word0,
    const uint32_t* __restrict__ chunk_off, uint32_t chunks, uint32_t first_block, uint32_t* __restrict__ index, uint64_t cap)
{
    __shared__ uint32_t wave_tot[4];
    const uint64_t w = word0 + (uint64_t)blockIdx.x * alloc::CHUNK_WORDS + threadIdx.x;
    uint32_t bits = alloc::word_bits(src, w, nbits, ds, src.B);
    uint32_t total;
    uint64_t at = block_excl_prefix((uint32_t)__builtin_popcount(bits), wave_tot, total);
    at += PPFS_DBG_OK(chunk_off + blockIdx.x, 4, chunk_off, (uint64_t)chunks * 4) ? chunk_off[blockIdx.x] : 0u;
    const uint32_t base = first_block + (uint32_t)(32u * w); // first_block + nbits <= 2^32 (the entry point)
    while (bits) {
        const uint32_t i = (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1u;
        if (at < cap && PPFS_DBG_OK(index + at, 4, index, cap * 4))
            index[at] = base + i;
        ++at;
    }
}

// index[i] = first + i: the bitmap's own blocks as a list
__global__ __launch_bounds__(256) void alloc_iota_kernel(uint32_t* __restrict__ index, uint32_t first, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && PPFS_DBG_OK(index + i, 4, index, n * 4))
        index[i] = first + (uint32_t)i;
}

// The statuses of a list decode, st[k] for entry index[k], k < n:
//   status_out (may be null; then index is not read): status_out[index[k] - first] = st[k] where that
//   lies below out_n -- the per-bit array of the allocated scrub, any alignment;
//   counts (may be null): counts[slot0 + alloc::count_slot(st[k])] grows by one for the slots below ncat.
// The tally is status_tally.hpp's, over the workgroup's strided share of the entries.
__global__ __launch_bounds__(256) void scrub_tally_kernel(const uint8_t* __restrict__ st, const uint32_t* __restrict__ index,
    uint64_t n, uint32_t first, uint8_t* __restrict__ status_out, uint64_t out_n, unsigned long long* __restrict__ counts,
    int slot0, int ncat)
{
    uint32_t c[4] = { 0, 0, 0, 0 };
    for (uint64_t k0 = (uint64_t)blockIdx.x * 256u; k0 < n; k0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t k = k0 + threadIdx.x;
        int slot = -1;
        if (k < n && PPFS_DBG_OK(st + k, 1, st, n)) {
            const uint32_t s = st[k];
            slot = alloc::count_slot(s);
            if (status_out && PPFS_DBG_OK(index + k, 4, index, n * 4)) {
                const uint32_t j = index[k] - first;
                if (j < out_n && PPFS_DBG_OK(status_out + j, 1, status_out, out_n))
                    status_out[j] = (uint8_t)s;
            }
        }
        tally_add(c, slot);
    }
    tally_flush(c, counts, slot0, ncat);
}

} // namespace ppfs

// One piece of the bitmap -> its ascending block list.  stream: 4-byte aligned, B * ds bytes; scratch:
// 2 * alloc::PIECE_CHUNKS dwords (chunk totals, chunk offsets); index: room for `bits` entries;
// *piece_total (8-byte aligned) receives the number written; counts (may be null): the record whose
// not_allocated grows by the piece's clear bits.
extern "C" hipError_t ppfs_alloc_expand_launch(const uint8_t* stream, const uint8_t* bstatus, uint64_t B, uint64_t ds,
    uint64_t nbits, uint32_t first_block, uint64_t piece, uint32_t* scratch, unsigned long long* piece_total, uint32_t* index,
    unsigned long long* counts, hipStream_t s)
{
    using namespace ppfs;
    if (ds == 0 || piece >= alloc::pieces_of(nbits) || ((uintptr_t)stream & 3u) || ((uintptr_t)piece_total & 7u)
        || ((uintptr_t)counts & 7u) || B != alloc::blocks_spanned(nbits, ds))
        return hipErrorInvalidValue;
    const alloc::Piece p = alloc::piece_of(nbits, piece);
    const AllocSrc src { stream, B * ds, bstatus, B };
    uint32_t *tot = scratch, *off = scratch + alloc::PIECE_CHUNKS;
    hipLaunchKernelGGL(alloc_count_kernel, dim3(p.chunks), dim3(256), 0, s, src, nbits, ds, p.word0, tot, p.chunks);
    hipLaunchKernelGGL(alloc_offsets_kernel, dim3(1), dim3(256), 0, s, tot, p.chunks, off, piece_total, p.bits, counts);
    hipLaunchKernelGGL(alloc_expand_kernel, dim3(p.chunks), dim3(256), 0, s, src, nbits, ds, p.word0, off, p.chunks,
        first_block, index, p.bits);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_alloc_iota_launch(uint32_t* index, uint32_t first, uint64_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const uint64_t grid = (n + 255u) / 256u;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ppfs::alloc_iota_kernel, dim3((uint32_t)grid), dim3(256), 0, s, index, first, n);
    return hipGetLastError();
}

// index and status_out go together (both or neither); slot0 / ncat: 0 / 4 for data blocks and list
// entries, alloc::SLOT_BITMAP / 3 for the bitmap's own blocks
extern "C" hipError_t ppfs_scrub_tally_launch(const uint8_t* st, const uint32_t* index, uint64_t n, uint32_t first,
    uint8_t* status_out, uint64_t out_n, unsigned long long* counts, int slot0, int ncat, hipStream_t s)
{
    if (n == 0 || (!status_out && !counts))
        return hipSuccess;
    if ((status_out && !index) || ((uintptr_t)counts & 7u) || slot0 < 0 || ncat < 0 || ncat > 4 || slot0 + ncat > 8)
        return hipErrorInvalidValue;
    const uint64_t want = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(want < 2048u ? want : 2048u);
    hipLaunchKernelGGL(ppfs::scrub_tally_kernel, dim3(grid), dim3(256), 0, s, st, status_out ? index : nullptr, n, first,
        status_out, out_n, counts, slot0, ncat);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_alloc_faults)
