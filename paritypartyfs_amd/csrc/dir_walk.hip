// dir_walk.hip -- the kernels of the directory lookups (lookup_path.cpp; include/ppfs_ecc.h ppfs_ecc_lookup_*).
//
// ppfs_ecc_read_files_* has left every directory's entries in the call's entries buffer, directory d at out_pos,
// entry e at out_pos + 128 e (no alignment), and one final status per file block.  Two kernels answer the queries:
//   lookup_match_kernel   one wave per (query, chunk of lookupplan::CHUNK entries).  The query's key is the wave's:
//                         lane j < 32 holds word j of the name record and every lane reads a word by v_readlane, so
//                         the key costs one VGPR and no LDS.  A lane takes one entry per step: its first 16 bytes
//                         (inode number and 12 name bytes) first, the other 112 only while the entry still agrees
//                         and only as far as the query's length reaches.  The wave's lowest matching entry comes
//                         from a ballot; lane 0 lowers the query's slot (the `entry` word of its hit record, set to
//                         0xFFFFFFFF on the stream before) with one 32-bit atomicMin, and the wave ends: what it
//                         would look at next lies behind.  A wave whose chunk starts behind the slot's value ends
//                         at once.
//   lookup_finish_kernel  one wave per query: B and last(B) from the slot, the lowest 5 / 9 among the directory's
//                         block statuses [block_pos, block_pos + last(B)] by ballot over 64 blocks a step, the hit
//                         record, the tally (status_tally.hpp).
// Loads.  Entries start at any byte, so all entry loads go through funnel.hpp's aligned dwords; neighbouring lanes
// are 128 bytes apart, one cache line each, which is why a lane fetches 16 bytes before it decides to fetch more.
// Every index is checked against its array's extent before use; the rule is lookup_plan.hpp's.  No scratch, no
// spills, no LDS beyond the tally's 64 bytes.
#include <hip/hip_runtime.h>

#include "dbg.hpp"
#include "funnel.hpp"
#include "kernels.hpp"
#include "lookup_plan.hpp"
#include "status_tally.hpp"
#include <stdint.h>

namespace ppfs {

using namespace lookupplan;

// the little-endian dword at p, any alignment, from the aligned dwords that hold its bytes
__device__ inline uint32_t load4_any(const uint8_t* p)
{
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* a = (const uint32_t*)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t w0 = a[0];
    return sh == 0 ? w0 : __builtin_amdgcn_alignbyte(a[1], w0, sh);
}

__device__ inline uint32_t pick4(const uint4& u, uint32_t i) { return i == 0 ? u.x : i == 1 ? u.y : i == 2 ? u.z : u.w; }

// waves_per_query waves share a query's chunks round robin.  hits: nq records of four dwords, dword 1 the slot
__global__ __launch_bounds__(256) void lookup_match_kernel(const DirRec* __restrict__ dirs, uint64_t ndirs, const Query* __restrict__ queries,
    const uint8_t* __restrict__ names, uint64_t nq, int mode, const uint8_t* __restrict__ entries, uint64_t entries_bytes,
    uint32_t waves_per_query, uint32_t* hits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint64_t q = wave / waves_per_query;
    if (q >= nq || !PPFS_DBG_OK(queries + q, 8, queries, nq * 8))
        return;
    const Query qr = queries[q];
    if (qr.dir >= ndirs || !PPFS_DBG_OK(dirs + qr.dir, 32, dirs, ndirs * 32))
        return;
    const DirRec d = dirs[qr.dir];
    uint32_t* slot = hits + 4u * q + 1u;
    if (!PPFS_DBG_OK(slot, 4, hits, nq * 16))
        return;

    // the key: lane j < 32 holds word j of the query's 128 name bytes (any alignment: byte loads, once per wave)
    uint32_t mine = 0, need = 0;
    if (mode == MODE_NAME) {
        const uint8_t* nm = names + QUERY_BYTES * q + 4u * (lane & 31u);
        if (PPFS_DBG_OK(nm, 4, names, nq * QUERY_BYTES))
            mine = (uint32_t)nm[0] | (uint32_t)nm[1] << 8 | (uint32_t)nm[2] << 16 | (uint32_t)nm[3] << 24;
        const uint32_t L = query_length([&](uint32_t w) { return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)w); });
        if (!query_usable(L))
            return; // matches nothing
        need = L + 1u;
    }
    const auto query_word = [&](uint32_t w) { return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)w); };
    const uint32_t tail_groups = need > 12u ? (need - 12u + 15u) / 16u : 0u; // 16-byte groups behind the first 16 bytes

    const uint64_t nchunks = chunks_of(d.n);
    for (uint64_t ch = wave % waves_per_query; ch < nchunks; ch += waves_per_query) {
        const uint64_t base = ch * CHUNK;
        if ((uint64_t)__atomic_load_n(slot, __ATOMIC_RELAXED) < base)
            return; // a match in front of this chunk is known: nothing here or behind can lower it
        for (uint32_t step = 0; step < CHUNK / 64u; ++step) {
            const uint64_t e = base + 64u * step + lane;
            const uint8_t* p = entries + d.out_pos + ENTRY_BYTES * e;
            bool hit = false;
            if (e < d.n && d.out_pos + ENTRY_BYTES * (e + 1u) <= entries_bytes && PPFS_DBG_OK(p, ENTRY_BYTES, entries, entries_bytes)) {
                if (mode == MODE_INODE) {
                    hit = inode_match(load4_any(p), qr.key);
                } else {
                    const uint4 head = load16_funnel(p); // word 0 the inode number, then name words 0..2
                    hit = words_agree([&](uint32_t w) { return pick4(head, w + 1u); }, query_word, 0u, 3u, need);
                    for (uint32_t g = 0; g < tail_groups; ++g) { // the bound is the wave's; a lane that differs loads no more
                        if (hit) {
                            const uint4 u = load16_funnel(p + 16u + 16u * g);
                            const uint32_t w0 = 3u + 4u * g;
                            hit = words_agree([&](uint32_t w) { return pick4(u, w - w0); }, query_word, w0, w0 + 4u, need);
                        }
                    }
                }
            }
            const unsigned long long found = __builtin_amdgcn_ballot_w64(hit);
            if (found) {
                if (lane == 0)
                    atomicMin(slot, (uint32_t)(base + 64u * step + (uint32_t)__builtin_ctzll(found)));
                return;
            }
        }
    }
}

// block_status: total_blocks final statuses; hits: nq records, dword 1 the slot the match kernel left
__global__ __launch_bounds__(256) void lookup_finish_kernel(const DirRec* __restrict__ dirs, uint64_t ndirs, const Query* __restrict__ queries,
    uint64_t nq, const uint8_t* __restrict__ entries, uint64_t entries_bytes, const uint8_t* __restrict__ block_status,
    uint64_t total_blocks, uint64_t ds, uint32_t* hits, unsigned long long* __restrict__ counts)
{
    uint32_t c[4] = { 0, 0, 0, 0 };
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t q0 = (uint64_t)blockIdx.x * 4u; q0 < nq; q0 += (uint64_t)gridDim.x * 4u) {
        const uint64_t q = q0 + (threadIdx.x >> 6);
        int tally = -1;
        if (q < nq && PPFS_DBG_OK(queries + q, 8, queries, nq * 8) && PPFS_DBG_OK(hits + 4u * q, 16, hits, nq * 16)) {
            const Query qr = queries[q];
            DirRec d { 0, 0, 0, 0 };
            if (qr.dir < ndirs && PPFS_DBG_OK(dirs + qr.dir, 32, dirs, ndirs * 32))
                d = dirs[qr.dir];
            const uint32_t m = hits[4u * q + 1u];
            uint32_t failure = 0;
            if (d.n && d.blocks) {
                uint64_t last = last_block(d.n, m, ds);
                last = last < d.blocks ? last : d.blocks - 1u;
                for (uint64_t j0 = 0; j0 <= last && !failure; j0 += 64u) {
                    const uint64_t at = d.block_pos + j0 + lane;
                    uint32_t s = 0;
                    if (j0 + lane <= last && at < total_blocks && PPFS_DBG_OK(block_status + at, 1, block_status, total_blocks))
                        s = block_status[at];
                    const unsigned long long bad = __builtin_amdgcn_ballot_w64(fails(s));
                    if (bad)
                        failure = (uint32_t)__builtin_amdgcn_readlane((int)s, __builtin_ctzll(bad));
                }
            }
            if (lane == 0) {
                uint32_t inode = NONE;
                const uint8_t* p = entries + d.out_pos + (uint64_t)ENTRY_BYTES * m;
                if (d.n && !failure && m != NONE && m < d.n && d.out_pos + (uint64_t)ENTRY_BYTES * (m + 1ull) <= entries_bytes
                    && PPFS_DBG_OK(p, 4, entries, entries_bytes))
                    inode = load4_any(p);
                const Hit h = answer(d.n, m < d.n ? m : NONE, failure, inode);
                hits[4u * q] = h.inode;
                hits[4u * q + 1u] = h.entry;
                hits[4u * q + 2u] = h.status;
                hits[4u * q + 3u] = 0u;
                tally = count_slot(h.status);
            }
        }
        tally_add(c, tally);
    }
    tally_flush(c, counts, 0, 4);
}

} // namespace ppfs

using namespace ppfs;

// The waves a query gets: one per chunk up to 8; longer directories are walked round robin, and a wave behind a
// known match ends at once.  The number is the call's, sized by its LONGEST directory: a query on a shorter one
// starts waves that find no chunk and leave after two loads.  One long directory among many short ones therefore
// launches mostly idle waves (at most 8 a query); per-query wave counts would need a prefix table built on the
// host, which was not built or measured
static uint32_t waves_per_query(uint64_t max_entries)
{
    const uint64_t chunks = chunks_of(max_entries);
    return (uint32_t)(chunks < 1u ? 1u : chunks < 8u ? chunks : 8u);
}

extern "C" hipError_t ppfs_lookup_match_launch(const void* dirs, uint64_t ndirs, const void* queries, const uint8_t* names,
    uint64_t nq, int mode, const uint8_t* entries, uint64_t entries_bytes, uint64_t max_entries, void* hits, hipStream_t s)
{
    if (nq == 0 || max_entries == 0)
        return hipSuccess;
    if (!dirs || !queries || !entries || !hits || (mode != MODE_NAME && mode != MODE_INODE) || (mode == MODE_NAME && !names)
        || (((uintptr_t)dirs | (uintptr_t)queries) & 7u) || ((uintptr_t)hits & 3u) || max_entries >= NONE)
        return hipErrorInvalidValue;
    const uint32_t wpq = waves_per_query(max_entries);
    const uint64_t grid = (nq * wpq + 3u) / 4u;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookup_match_kernel, dim3((uint32_t)grid), dim3(256), 0, s, (const DirRec*)dirs, ndirs, (const Query*)queries, names,
        nq, mode, entries, entries_bytes, wpq, (uint32_t*)hits);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_lookup_finish_launch(const void* dirs, uint64_t ndirs, const void* queries, uint64_t nq,
    const uint8_t* entries, uint64_t entries_bytes, const uint8_t* block_status, uint64_t total_blocks, uint64_t ds, void* hits,
    unsigned long long* counts, hipStream_t s)
{
    if (nq == 0)
        return hipSuccess;
    if (!dirs || !queries || !hits || ds == 0 || (((uintptr_t)dirs | (uintptr_t)queries | (uintptr_t)counts) & 7u)
        || ((uintptr_t)hits & 3u) || (total_blocks && (!entries || !block_status)))
        return hipErrorInvalidValue;
    const uint64_t want = (nq + 3u) / 4u;
    hipLaunchKernelGGL(lookup_finish_kernel, dim3((uint32_t)(want < 4096u ? want : 4096u)), dim3(256), 0, s, (const DirRec*)dirs, ndirs,
        (const Query*)queries, nq, entries, entries_bytes, block_status, total_blocks, ds, (uint32_t*)hits, counts);
    return hipGetLastError();
}

// this unit's PPFS_ECC_DEBUG counter, summed into ppfs_ecc_debug_faults (api.cpp)
PPFS_DBG_ACCESSOR(ppfs_dbg_lookup_faults)
