// extent_plan.hpp -- the arithmetic of the byte-extent calls (extent_path.cpp), over plain numbers
// and bytes: the clamp of an entry's length, the validity of an entry, the index an entry is staged
// under, the layout of the calls' second staging, the CPU pack / overlay of the host forms and the
// entries of a readFile / writeFile walk.  No HIP and no context: tests/cpp/test_extent_plan.cpp
// checks it with the host compiler alone.  The cut of a host list into runs is list_plan.hpp's
// run_end over the staged indices.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ppfs_ecc.h"
#include "list_plan.hpp"

#pragma GCC visibility push(hidden) // nothing of this is part of the library's ABI
namespace ppfs {
namespace extplan {

constexpr uint32_t kNoBlock = 0xFFFFFFFFu; // the staged index of an invalid entry: out of range for every image

// The extent calls address blocks below 2^32 - 1: kNoBlock never names a block, so the list kernels
// (gather, scatter, range marks) treat an invalid entry as an out-of-range one with no new case.
inline size_t image_blocks_seen(size_t image_blocks) { return std::min<size_t>(image_blocks, kNoBlock); }

// min(length, dataSize() - offset): the clamp readBlock / writeBlock apply (rs_block_device.cpp:25-93,
// crc_block_device.cpp:69-122, hamming_block_device.cpp:111-162, parity_block_device.cpp:31-88).
// offset == ds is an access of zero bytes; offset > ds is no access at all (0 here, and invalid).
inline uint32_t eff_len(uint32_t offset, uint32_t length, size_t ds)
{
    if ((size_t)offset >= ds)
        return 0;
    return (uint32_t)std::min<size_t>(length, ds - offset);
}

// An entry is valid when its block is in the image, its offset is at most ds and its clamped bytes
// lie inside the packed caller buffer of buf_bytes.
inline bool valid(const ppfs_ecc_extent& e, size_t image_blocks, size_t ds, size_t buf_bytes)
{
    if ((uint64_t)e.block >= (uint64_t)image_blocks_seen(image_blocks) || (size_t)e.offset > ds)
        return false;
    const uint64_t len = eff_len(e.offset, e.length, ds);
    return e.pos <= (uint64_t)buf_bytes && len <= (uint64_t)buf_bytes - e.pos;
}

inline uint32_t staged_index(const ppfs_ecc_extent& e, size_t image_blocks, size_t ds, size_t buf_bytes)
{
    return valid(e, image_blocks, ds, buf_bytes) ? e.block : kNoBlock;
}

// Bytes of the extent calls' own staging: the decoded payloads of one piece (rounded up: the copy
// kernel reads whole aligned dwords, the codecs store whole 16-byte windows), then the staged index
// of every entry of the piece.
struct ExtStageLayout {
    size_t payload, index, total;
};
inline ExtStageLayout ext_stage_layout(size_t piece, size_t ds)
{
    ExtStageLayout L {};
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    L.payload = 0;
    L.index = al(std::max<size_t>(piece * ds, 16));
    L.total = al(L.index + piece * 4);
    return L;
}

// out[pos, pos + len) = payload i's bytes [offset, offset + len) for the m entries of a run, zeros
// where the entry's status is 5; an entry staged as kNoBlock is skipped.  P holds the run's payloads
// at stride ds.
inline void pack_cpu(const uint8_t* P, size_t ds, const ppfs_ecc_extent* ext, const uint32_t* staged, const uint8_t* status,
    size_t m, uint8_t* out)
{
    for (size_t i = 0; i < m; ++i) {
        if (staged[i] == kNoBlock)
            continue;
        const uint32_t len = eff_len(ext[i].offset, ext[i].length, ds);
        if (!len)
            continue;
        if (status && status[i] == listplan::kCorrectionError)
            std::memset(out + ext[i].pos, 0, len);
        else
            std::memcpy(out + ext[i].pos, P + i * ds + ext[i].offset, len);
    }
}

// payload i's bytes [offset, offset + len) = in[pos, pos + len), same rules
inline void overlay_cpu(const uint8_t* in, const ppfs_ecc_extent* ext, const uint32_t* staged, size_t m, uint8_t* P, size_t ds)
{
    for (size_t i = 0; i < m; ++i) {
        if (staged[i] == kNoBlock)
            continue;
        const uint32_t len = eff_len(ext[i].offset, ext[i].length, ds);
        if (len)
            std::memcpy(P + i * ds + ext[i].offset, in + ext[i].pos, len);
    }
}

// The entries of FileIO::readFile / writeFile (file_io.cpp:24-42, 50-88) for nbytes of a file whose
// blocks, from the one that holds the first byte on, are indices[0 .. n): the first block from
// off0 = offset % dataSize(), whole blocks after it, the last one up to where the bytes run out;
// pos is the running sum, so the packed buffer is the file range itself.  Stops when the bytes or
// the blocks run out; returns the bytes covered.
inline size_t file_extents(const uint32_t* indices, size_t n, size_t off0, size_t nbytes, size_t ds,
    std::vector<ppfs_ecc_extent>& out)
{
    out.clear();
    size_t done = 0;
    if (ds == 0 || off0 >= ds)
        return 0;
    for (size_t k = 0; k < n && done < nbytes; ++k) {
        const size_t off = k == 0 ? off0 : 0;
        const size_t len = std::min(ds - off, nbytes - done);
        out.push_back(ppfs_ecc_extent { (uint64_t)done, indices[k], (uint16_t)off, (uint16_t)len });
        done += len;
    }
    return done;
}

} // namespace extplan
} // namespace ppfs
#pragma GCC visibility pop
