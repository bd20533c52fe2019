// list_plan.hpp -- the arithmetic of the block-list calls (list_path.cpp), over plain numbers and
// bytes: the range check of an entry, the pieces of a device list call, the cut of a host list into
// runs without a repeated index, the CPU row gather and the choice of rows a run copies back.  No HIP
// and no context: tests/cpp/test_list_plan.cpp checks it with the host compiler alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

#pragma GCC visibility push(hidden) // nothing of this is part of the library's ABI
namespace ppfs {
namespace listplan {

constexpr uint8_t kOk = 0, kCorrected = 1, kCorrectionError = 5, kOutOfBounds = 9; // enum ppfs_ecc_status

enum Op { OP_DECODE = 0, OP_ENCODE = 1, OP_WRITE = 2 };

// An index is a block of the image when it is below image_blocks; the list's indices are unsigned
// 32-bit, so a caller's -1 is 0xFFFFFFFF and out of range for every image of fewer than 2^32 blocks.
inline bool in_range(uint32_t index, size_t image_blocks) { return (uint64_t)index < (uint64_t)image_blocks; }

// Blocks per piece of a device list call: the host chunk size rounded down to a multiple of 1 Ki
// (so a piece's payload and status offsets keep the caller's 16-byte alignment), at least 1 Ki, and
// small enough that a piece's bytes stay below 2^31 (the list kernels count bytes in 32 bits).
inline size_t piece_blocks(size_t chunk_blocks, size_t raw)
{
    const size_t cap = std::max<size_t>(1024, (((size_t)1 << 31) / std::max<size_t>(raw, 1)) & ~(size_t)1023);
    return std::min(cap, std::max<size_t>(1024, chunk_blocks & ~(size_t)1023));
}

// Bytes of the context's list staging: the rows of one piece, rounded up (the kernels store and read
// whole 16-byte windows), then one status byte per block.
struct StageLayout {
    size_t rows, status, total;
};
inline StageLayout stage_layout(size_t piece, size_t raw)
{
    StageLayout L {};
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    L.rows = 0;
    L.status = al(piece * raw);
    L.total = al(L.status + piece);
    return L;
}

// The end of the run that starts at list position `start`: the longest stretch [start, end) of at
// most max_run entries in which no in-range index repeats.  Out-of-range entries never end a run:
// they touch no block.  The host calls process run after run, so that a block listed twice is seen
// by its second entry as its first entry left it -- the per-block calls made in list order.
inline size_t run_end(const uint32_t* index, size_t n, size_t start, size_t image_blocks, size_t max_run)
{
    std::unordered_set<uint32_t> seen;
    size_t e = start;
    const size_t stop = std::min(n, start + std::max<size_t>(max_run, 1));
    for (; e < stop; ++e) {
        if (!in_range(index[e], image_blocks))
            continue;
        if (!seen.insert(index[e]).second)
            break;
    }
    return e;
}

// rows[i] = image row index[i] for the m entries of a run (zeros for an out-of-range entry)
inline void gather_rows_cpu(const uint8_t* image, size_t image_blocks, const uint32_t* index, size_t m, size_t raw,
    uint8_t* rows)
{
    for (size_t i = 0; i < m; ++i) {
        if (in_range(index[i], image_blocks))
            std::memcpy(rows + i * raw, image + (size_t)index[i] * raw, raw);
        else
            std::memset(rows + i * raw, 0, raw);
    }
}

// Does entry i of a finished run go back into the image?  decode: the rows its write-back changed
// (status 1); write: every row whose old block passed its check (status other than 5); encode:
// every row.  Never an out-of-range entry.
inline bool copies_back(Op op, bool write_back, uint32_t index, size_t image_blocks, uint8_t status)
{
    if (!in_range(index, image_blocks))
        return false;
    switch (op) {
    case OP_DECODE:
        return write_back && status == kCorrected;
    case OP_WRITE:
        return status != kCorrectionError;
    case OP_ENCODE:
        return true;
    }
    return false;
}

// The run's rows that go back, ascending (positions inside the run)
inline std::vector<uint32_t> copy_back_list(Op op, bool write_back, const uint32_t* index, size_t m, size_t image_blocks,
    const uint8_t* status)
{
    std::vector<uint32_t> out;
    for (size_t i = 0; i < m; ++i)
        if (copies_back(op, write_back, index[i], image_blocks, status ? status[i] : kOk))
            out.push_back((uint32_t)i);
    return out;
}

// What an out-of-range entry reports: status 9 and a zero payload
inline void mark_out_of_range(const uint32_t* index, size_t m, size_t image_blocks, uint8_t* status, uint8_t* data,
    size_t data_bytes)
{
    for (size_t i = 0; i < m; ++i) {
        if (in_range(index[i], image_blocks))
            continue;
        if (status)
            status[i] = kOutOfBounds;
        if (data && data_bytes)
            std::memset(data + i * data_bytes, 0, data_bytes);
    }
}

} // namespace listplan
} // namespace ppfs
#pragma GCC visibility pop
