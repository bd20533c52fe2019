// resident_plan.hpp -- how much of a batch's codeword image the RS 2t <= 8 ticket encode
// (rs_wg_tk.hpp) leaves cache-resident: the first res_tiles 64-block tiles of the batch.  Plain numbers,
// no HIP and no context: tests/cpp/test_resident_plan.cpp checks it with the host compiler alone.
//
// The policy is per call: an encode launch gets res_tiles from the context it goes through and the
// batch it is given; nothing is remembered between calls and no other call reads the setting.  So
// nothing happens when the encode and the decode (or scrub, or injection) of an image go through
// different contexts: whoever touches the codewords next finds the prefix in the cache or does not,
// which changes its speed and never a result.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#pragma GCC visibility push(hidden) // nothing of this is part of the library's ABI
namespace ppfs {
namespace plan {

constexpr uint64_t kResidentTileBytes = 64u * 255u; // one tile of codewords (n = 255 for every fast code)

// Default prefix, bytes: 255 MiB, the largest setting of the sweep in DESIGN.md Appendix A ("resident
// prefix": the step gets faster with every setting up to it, no kernel falls off).  0 would be off:
// every tile streams, as before the prefix existed.
constexpr uint64_t kResidentBytesDefault = 255ull << 20;

// PPFS_ECC_RESIDENT_MIB, read once when a context is created: the prefix in MiB (a decimal fraction
// is allowed), 0 = off.  Unset, empty, negative or not a number: the default.
inline uint64_t resident_env(const char* e, uint64_t dflt = kResidentBytesDefault)
{
    if (!e || !*e)
        return dflt;
    char* end = nullptr;
    const double v = std::strtod(e, &end);
    if (end == e || *end || !std::isfinite(v) || v < 0.0)
        return dflt;
    return (uint64_t)(std::min(v, 1048576.0) * 1048576.0); // at most 1 TiB: no overflow, past any cache
}

// Tiles of an nblocks batch that form the resident prefix.  The place to cap a batch's prefix.
inline uint64_t resident_tiles(uint64_t nblocks, uint64_t resident_bytes)
{
    const uint64_t ntiles = nblocks / 64u + (nblocks % 64u ? 1u : 0u);
    return std::min(ntiles, resident_bytes / kResidentTileBytes);
}

} // namespace plan
} // namespace ppfs
#pragma GCC visibility pop
