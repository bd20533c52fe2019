// host_plan.hpp -- the arithmetic of the chunked host path (host_path.cpp), over plain numbers and
// bytes: chunk sizes, the staging layout, the scan of a chunk's status for changed blocks and the
// application of a patch list.  No HIP and no context: tests/cpp/test_host_plan.cpp checks it with
// the host compiler alone.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <vector>

#include "host_copy.hpp"

#pragma GCC visibility push(hidden) // nothing of this is part of the library's ABI
namespace ppfs {
namespace plan {

// 16 MiB of codewords per chunk: 64 Ki RS(255, k) blocks (round 6, r6e: page-locked encode / 1-error
// decode 75.9-76.1 / 42.9-43.1 GiB/s vs 71.9-72.1 / 40.9-41.0 at 32 Ki, 98-262 Ki no better), 4 Ki
// blocks of 4 KiB
constexpr size_t kChunkBytes = 16u << 20;

// PPFS_ECC_CHUNK_BLOCKS (1 Ki .. 4 Mi): another chunk size (the r6e sweep); 0 = unset or out of range
inline size_t chunk_env(const char* e)
{
    const long v = e ? std::atol(e) : 0;
    return v >= 1024 && v <= (1l << 22) ? (size_t)v : 0;
}
// Blocks per chunk of a context's host calls: the override, else a multiple of 1 Ki, at least 1 Ki
inline size_t chunk_blocks(size_t raw, size_t env)
{
    return env ? env : std::max<size_t>(1024, (kChunkBytes / std::max<size_t>(raw, 1)) & ~(size_t)1023);
}

// Chunk sizes of a pipelined host call of at least 8 chunks: the first chunks ramp up (chunk / 8,
// / 4, / 2) and the last ones ramp down (halving the remainder), so the pipeline's fill (the first
// H2D before any kernel or D2H) and drain (the last D2H with no H2D beside it) move small chunks,
// not whole ones.  r6g (page-locked, 2 rounds x 7 reps): clean decode 70.3-72.3 vs 64.0-65.3 GiB/s,
// 1-error decode 41.6-42.6 vs 41.3-42.7, encode 71.5-75.4 vs 71.6-76.1.  (Four staging slots
// instead of three: encode 51-52, decode 31-37 GiB/s; a decode's codewords returned on the H2D
// stream: 26 GiB/s -- both dropped.)
// Never more than `chunk`, which the staging is laid out for: with a chunk that is no multiple of
// 1 Ki, or below 8 Ki, the rounding and the no-small-tail rule below would otherwise exceed it.
inline size_t ramp_chunk(size_t index, size_t remaining, size_t chunk)
{
    const size_t least = std::max<size_t>(chunk / 8, 1024);
    size_t nb = chunk;
    if (index < 3)
        nb = std::max(least, chunk >> (3 - index));
    if (remaining < 2 * nb) // ramp down: half of what is left (at least `least`)
        nb = std::max(least, (remaining / 2 + 1023) & ~(size_t)1023);
    nb = remaining < nb + least ? remaining : nb; // no piece smaller than `least` after it
    return std::min(nb, chunk);
}

// The pieces of one host call, in order.  `chunk` = min(nblocks, the context's chunk size) is what
// the staging is laid out for; calls shorter than 8 chunks go in whole chunks and a remainder.
struct ChunkSeq {
    size_t nblocks, chunk, index = 0, done = 0;
    ChunkSeq(size_t nblocks_, size_t chunk_blocks_) : nblocks(nblocks_), chunk(std::min(nblocks_, chunk_blocks_)) {}
    size_t next() // 0: the call is through
    {
        const size_t left = nblocks - done;
        const size_t nb = nblocks >= 8 * chunk ? ramp_chunk(index, left, chunk) : std::min(chunk, left);
        ++index;
        done += nb;
        return nb;
    }
};

// a decode with write-back returns only the codewords it changed (status 1): as a packed gather
// when at most nb / kGatherDiv blocks changed, else the chunk's whole codeword range
constexpr size_t kGatherDiv = 8;
inline size_t gather_rows(size_t nb) { return nb / kGatherDiv + 1; } // rows of the idx and gat regions

// a decode's spill record per block: the count and the bytes a shortened RS code's write-back puts
// past the block end (1 byte for every other codec)
inline size_t spill_bytes(size_t raw) { return 256 - std::min<size_t>(raw, 255); }

struct Layout { // offsets inside one staging buffer
    size_t data, raw, status, spill, idx, gat, orig, patch, total;
};

// patch_slots: slots per block of a decode's patch list (0: the codec returns whole codewords)
inline Layout layout_for(size_t data, size_t raw, uint32_t patch_slots, size_t nb)
{
    Layout L {};
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    L.data = 0;
    L.raw = al(L.data + nb * data);
    L.status = al(L.raw + nb * raw);
    L.spill = al(L.status + nb);
    L.idx = al(L.spill + nb * spill_bytes(raw));
    L.gat = al(L.idx + gather_rows(nb) * sizeof(uint32_t));
    L.orig = al(L.gat + gather_rows(nb) * raw);
    L.patch = al(L.orig + (patch_slots ? nb * raw : 0));
    L.total = al(L.patch + nb * patch_slots * sizeof(uint32_t));
    return L;
}

// The changed blocks (status 1) of a landed chunk: their count, the first gather_rows(nb) of them
// in ix (nullptr: count only), and the predictor's verdict -- many changed, so the next chunks'
// codewords are fetched eagerly (queued behind the kernel) instead of after the status has landed
struct Changed {
    size_t count;
    bool eager;
};
inline Changed scan_changed(const uint8_t* sts, size_t nb, uint32_t* ix)
{
    size_t nchg = 0;
    for (size_t b = 0; b < nb; ++b)
        if (sts[b] == 1) {
            if (ix && nchg <= nb / kGatherDiv)
                ix[nchg] = (uint32_t)b;
            ++nchg;
        }
    return Changed { nchg, nchg > nb / kGatherDiv };
}

// patch list (vote.hip patch_list_kernel): S slots per block, each (offset << 8) | byte
constexpr uint32_t kPatchEnd = 0xFFFFFFFFu; // no further slot of this block is used
constexpr uint32_t kPatchOverflow = 0xFFFFFFFEu; // in slot 0: more than S bytes changed
constexpr size_t kPatchPart = 4096; // blocks per pool item

// worth the pool: several parts, many changed blocks (nchg), and a pool to run on
inline bool patch_pooled(size_t nb, size_t nchg)
{
    return nb > kPatchPart && nchg > 4 * kPatchPart && !g_fork_child.load(std::memory_order_relaxed) && copy_threads() > 1;
}

// Writes the changed bytes of the status-1 blocks into img (nb blocks of n bytes).  Returns the
// blocks that overflowed their slots, ascending: those come back whole.
inline std::vector<uint32_t> apply_patch_list(uint8_t* img, size_t n, const uint8_t* sts, const uint32_t* P, uint32_t S,
    size_t nb, bool pooled)
{
    std::atomic<bool> overflow { false };
    const std::function<void(size_t)> part = [&](size_t p) {
        const size_t e = std::min(nb, (p + 1) * kPatchPart);
        for (size_t b = p * kPatchPart; b < e; ++b) {
            if (sts[b] != 1)
                continue;
            const uint32_t* q = P + b * S;
            if (q[0] == kPatchOverflow) {
                overflow.store(true, std::memory_order_relaxed);
                continue;
            }
            for (uint32_t j = 0; j < S && q[j] != kPatchEnd; ++j)
                img[b * n + (q[j] >> 8)] = (uint8_t)q[j];
        }
    };
    const size_t parts = (nb + kPatchPart - 1) / kPatchPart;
    if (pooled)
        CopyPool::get().run_for(parts, part);
    else
        for (size_t p = 0; p < parts; ++p)
            part(p);
    std::vector<uint32_t> over;
    if (overflow.load())
        for (size_t b = 0; b < nb; ++b)
            if (sts[b] == 1 && P[b * S] == kPatchOverflow)
                over.push_back((uint32_t)b);
    return over;
}

} // namespace plan
} // namespace ppfs
#pragma GCC visibility pop
