#pragma once
// status_tally.hpp -- the tally of statuses into a 64-byte counts record that the merges of the file walk
// (files_walk.hip) and the scrub (alloc_scan.hip) share.  A workgroup of 256 lanes walks its share of the entries,
// every lane with the slot of its entry (-1: none); each category is counted by wave ballot and popcount, the
// four waves combine through LDS, and one lane per category adds the workgroup's sum with one 64-bit atomicAdd
// (none for a zero).  The record was zeroed on the stream before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbg.hpp"

namespace ppfs {

// one pass of the workgroup: every lane of the wave calls, with or without an entry
__device__ inline void tally_add(uint32_t (&c)[4], int slot)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
        c[q] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(slot == q));
}

// after the last pass, every lane of the workgroup: counts[slot0 + q] += the workgroup's c[q] for q < ncat
// (counts null: nothing, for the whole grid)
__device__ inline void tally_flush(const uint32_t (&c)[4], unsigned long long* __restrict__ counts, int slot0, int ncat)
{
    __shared__ uint32_t part[4][4];
    if (!counts)
        return;
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            part[threadIdx.x >> 6][q] = c[q];
    }
    __syncthreads();
    if (threadIdx.x < 4u && (int)threadIdx.x < ncat) {
        const uint32_t q = threadIdx.x;
        const unsigned long long sum = (unsigned long long)part[0][q] + part[1][q] + part[2][q] + part[3][q];
        if (sum && PPFS_DBG_OK(counts + slot0 + q, 8, counts, 64))
            atomicAdd(counts + slot0 + q, sum);
    }
}

} // namespace ppfs
