// vote.hip -- 2-of-3 bitwise majority of replicated records.
//
// Reference: SuperBlockManager::_performBitVoting, lib/super_block_manager/src/
// super_block_manager.cpp:133-165: for every bit of the record, majority = (b1 + b2 + b3 >= 2);
// copy k is "damaged" when any of its bits differs from the majority.  PPFS votes over the three
// SuperBlock copies at mount; the batched form here votes nrec records at once (any record size),
// one thread per byte: out = (a & b) | (a & c) | (b & c) as one v_bitop3, and a record's damage
// bits are set with one atomic OR only where a byte disagrees.
#include <hip/hip_runtime.h>

#include "../../include/ppfs_ecc.h" // ppfs_ecc_extent
#include "dbg.hpp"
#include "funnel.hpp"
#include <stdint.h>

namespace ppfs {

__global__ __launch_bounds__(256) void vote3_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ c, uint8_t* __restrict__ out, uint64_t rec_bytes, uint64_t nbytes,
    uint32_t* __restrict__ damaged)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes; i += stride) {
        const uint32_t x = a[i], y = b[i], z = c[i];
        const uint32_t m = __builtin_amdgcn_bitop3_b32(x, y, z, 0xE8); // majority
        out[i] = (uint8_t)m;
        const uint32_t bad = (x != m ? 1u : 0u) | (y != m ? 2u : 0u) | (z != m ? 4u : 0u);
        if (bad && damaged)
            atomicOr(&damaged[i / rec_bytes], bad);
    }
}

} // namespace ppfs

extern "C" hipError_t ppfs_vote3_launch(const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out,
    uint64_t rec_bytes, uint64_t nrec, uint32_t* damaged, hipStream_t s)
{
    const uint64_t nbytes = rec_bytes * nrec;
    if (damaged) {
        const hipError_t e = hipMemsetAsync(damaged, 0, nrec * sizeof(uint32_t), s);
        if (e != hipSuccess)
            return e;
    }
    if (nbytes == 0)
        return hipSuccess;
    const uint64_t want = (nbytes + 255) / 256;
    const uint32_t grid = (uint32_t)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(ppfs::vote3_kernel, dim3(grid), dim3(256), 0, s, a, b, c, out, rec_bytes, nbytes, damaged);
    return hipGetLastError();
}

// ---- gather of the rows a host decode has to return (host_path.cpp gather_rows_back) ----
// dst row i = src row idx[i] (row_bytes each): the codewords a decode with write-back changed
// (status 1), packed for one D2H copy when they are few.  One workgroup per row, 16-byte pieces
// where source and destination are 16-byte aligned, else bytes.
namespace ppfs {
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint8_t* __restrict__ src, [[maybe_unused]] uint64_t src_rows,
    uint8_t* __restrict__ dst, const uint32_t* __restrict__ idx, uint32_t nrows, uint32_t row_bytes)
{
    for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const uint8_t* s = src + (uint64_t)idx[r] * row_bytes;
        uint8_t* d = dst + (uint64_t)r * row_bytes;
        if (!PPFS_DBG_OK(s, row_bytes, src, src_rows * row_bytes) || !PPFS_DBG_OK(d, row_bytes, dst, (uint64_t)nrows * row_bytes))
            continue;
        if ((((uintptr_t)s | (uintptr_t)d | row_bytes) & 15u) == 0) {
            for (uint32_t p = threadIdx.x; 16u * p < row_bytes; p += blockDim.x)
                *(uint4*)(d + 16u * p) = *(const uint4*)(s + 16u * p);
        } else {
            for (uint32_t b = threadIdx.x; b < row_bytes; b += blockDim.x)
                d[b] = s[b];
        }
    }
}
} // namespace ppfs

// ---- patch list of a decode's write-back (host_path.cpp ChunkPipeline) ----
// The bytes a decode with write-back changed, for the host to patch into its image instead of
// copying every changed codeword back: block b with status[b] == 1 gets (pos << 8 | byte) for each
// byte where cur differs from orig (the codeword before the decode) in patch[b S .. b S + S - 1],
// in position order, its unused slots ~0; a block with more than S changed bytes gets 0xFFFFFFFE in
// slot 0 (the host fetches that codeword whole).  Other blocks' slots are not written.  With
// `image` (a device pointer to the caller's page-locked image, row b at image + b n) the changed
// bytes are stored there instead, over the link, and no list is made.  One wave per block, byte
// loads coalesced across the lanes, a ballot prefix for the slot of each change.
namespace ppfs {
__global__ __launch_bounds__(256) void patch_list_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ orig,
    const uint8_t* __restrict__ status, uint32_t n, uint64_t nb, uint32_t S, uint32_t* __restrict__ patch,
    uint8_t* __restrict__ image)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t b = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < nb; b += nw) {
        if (!PPFS_DBG_OK(status + b, 1, status, nb) || status[b] != 1)
            continue;
        const uint8_t* c = cur + b * n;
        const uint8_t* o = orig + b * n;
        uint32_t* slot = patch + b * S;
        uint32_t cnt = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
            const uint32_t j = j0 + lane;
            const uint32_t cv = j < n && PPFS_DBG_OK(c + j, 1, cur, nb * n) ? c[j] : 0u;
            const uint32_t ov = j < n && PPFS_DBG_OK(o + j, 1, orig, nb * n) ? o[j] : 0u;
            const bool d = j < n && cv != ov;
            if (image) {
                if (d)
                    image[b * n + j] = (uint8_t)cv;
                continue;
            }
            const uint64_t m = __builtin_amdgcn_ballot_w64(d);
            const uint32_t idx = cnt + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (d && idx < S && PPFS_DBG_OK(slot + idx, 4, patch, nb * S * 4))
                slot[idx] = j << 8 | cv;
            cnt += (uint32_t)__builtin_popcountll(m);
        }
        if (image)
            continue;
        if (cnt > S) {
            if (lane == 0 && PPFS_DBG_OK(slot, 4, patch, nb * S * 4))
                slot[0] = 0xFFFFFFFEu;
        } else {
            for (uint32_t j = cnt + lane; j < S; j += 64u)
                if (PPFS_DBG_OK(slot + j, 4, patch, nb * S * 4))
                    slot[j] = 0xFFFFFFFFu;
        }
    }
}
} // namespace ppfs

extern "C" hipError_t ppfs_patch_list_launch(const uint8_t* cur, const uint8_t* orig, const uint8_t* status, uint32_t n,
    uint64_t nb, uint32_t S, uint32_t* patch, uint8_t* image, hipStream_t s)
{
    if (nb == 0)
        return hipSuccess;
    const uint64_t want = (nb + 3) / 4;
    const uint32_t grid = (uint32_t)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(ppfs::patch_list_kernel, dim3(grid), dim3(256), 0, s, cur, orig, status, n, nb, S, patch, image);
    return hipGetLastError();
}

// ---- device copy at the HBM ceiling (measurement reference for bench.py's roofline) ----
// One thread per 16 bytes over a full grid (workgroups dispatched in address order: one
// contiguous window of HBM in flight), plain 16-byte loads and stores; ragged ends by bytes.
// The same shape reached 6.26 TB/s on 8.6 GB (tools/probes/stream_ablate4.hip).
namespace ppfs {
__global__ __launch_bounds__(256) void copy16_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
    uint64_t n16, uint64_t head, uint64_t bytes)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16)
        *(uint4*)(dst + head + 16 * i) = *(const uint4*)(src + head + 16 * i);
    if (i < head)
        dst[i] = src[i];
    const uint64_t tail0 = head + 16 * n16;
    if (i < bytes - tail0)
        dst[tail0 + i] = src[tail0 + i];
}
} // namespace ppfs

extern "C" hipError_t ppfs_copy_launch(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t s)
{
    if (bytes == 0)
        return hipSuccess;
    // 16-byte body where src and dst share their alignment, bytes elsewhere
    uint64_t head = ((uintptr_t)src ^ (uintptr_t)dst) & 15u ? bytes : ((16u - ((uintptr_t)src & 15u)) & 15u);
    if (head > bytes)
        head = bytes;
    const uint64_t n16 = (bytes - head) / 16;
    const uint64_t tail = bytes - head - 16 * n16;
    const uint64_t work = n16 > head ? (n16 > tail ? n16 : tail) : (head > tail ? head : tail);
    const uint64_t grid = (work + 255) / 256;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ppfs::copy16_kernel, dim3((uint32_t)grid), dim3(256), 0, s, dst, src, n16, head, bytes);
    return hipGetLastError();
}

// ---- fault injection: one byte per block (bench step, tests) ----
// Block b of a raw image at `stride` bytes per block gets byte pos[b] replaced by val[b] (mode 0)
// or XORed with it (mode 1); pos[b] >= stride skips the block.  The counterpart of the
// reference's bit flipper (usage_simulator/simulation/src/bit_flipper.cpp), used by bench.py to
// corrupt every codeword of a step: torch's index_put_ of the same bytes reads 8-byte indices and
// costs ~2x this kernel.  Each thread takes 4 consecutive blocks: one
// 4-byte load of their positions and one of their values, then four byte stores.  (Round 4: store
// instructions over 64 consecutive blocks instead, 16 KiB spans: 33 vs 30 us, r4zj; 8 or 16 blocks
// per thread with byte loads: 31.3 vs 30.0 us, r4zk; round 5: non-temporal byte stores and the
// blocks in reverse order, no gain, r5k.)
namespace ppfs {
template <int MODE>
__global__ __launch_bounds__(256) void inject_kernel(uint8_t* __restrict__ raw, uint64_t stride, uint64_t nblocks,
    const uint8_t* __restrict__ pos, const uint8_t* __restrict__ val)
{
    const uint64_t nq = (nblocks + 3) / 4, qi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq)
        return;
    const uint64_t b0 = 4 * qi;
    uint32_t p4, v4;
    if (b0 + 4 <= nblocks && ((uintptr_t)(pos + b0) & 3u) == 0 && ((uintptr_t)(val + b0) & 3u) == 0) {
        p4 = *(const uint32_t*)(pos + b0);
        v4 = *(const uint32_t*)(val + b0);
    } else {
        p4 = v4 = 0xFFFFFFFFu;
        for (uint64_t j = 0; j < 4 && b0 + j < nblocks; ++j) {
            p4 = (p4 & ~(0xFFu << (8 * j))) | ((uint32_t)pos[b0 + j] << (8 * j));
            v4 = (v4 & ~(0xFFu << (8 * j))) | ((uint32_t)val[b0 + j] << (8 * j));
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t p = (p4 >> (8 * j)) & 0xFFu;
        if (b0 + j >= nblocks || p >= stride)
            continue;
        uint8_t* d = raw + (b0 + j) * stride + p;
        const uint8_t v = (uint8_t)(v4 >> (8 * j));
        const uint8_t w = MODE == 0 ? v : (uint8_t)(*d ^ v);
        *d = w;
    }
}
} // namespace ppfs

extern "C" hipError_t ppfs_inject_launch(uint8_t* raw, uint64_t stride, uint64_t nblocks, const uint8_t* pos,
    const uint8_t* val, int mode, hipStream_t s)
{
    if (nblocks == 0)
        return hipSuccess;
    const uint64_t grid = ((nblocks + 3) / 4 + 255) / 256;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    if (mode == 0)
        hipLaunchKernelGGL(ppfs::inject_kernel<0>, dim3((uint32_t)grid), dim3(256), 0, s, raw, stride, nblocks, pos, val);
    else
        hipLaunchKernelGGL(ppfs::inject_kernel<1>, dim3((uint32_t)grid), dim3(256), 0, s, raw, stride, nblocks, pos, val);
    return hipGetLastError();
}

// Completion flag of the small-batch launch path (host_path.cpp wait_flag): queued after a call's
// kernels on the same stream, it makes their outputs visible system-wide and stores `v` (release)
// into host-coherent memory, where the host spins on it.  Cheaper than hipStreamSynchronize's
// completion signal (measured 6.4 vs 10.3 us for one empty kernel, tools/probes/latency_probe.cpp).
namespace ppfs {
__global__ __launch_bounds__(64) void flag_kernel(uint32_t* flag, uint32_t v)
{
    __threadfence_system();
    if (threadIdx.x == 0)
        __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
} // namespace ppfs

extern "C" hipError_t ppfs_flag_launch(uint32_t* flag, uint32_t v, hipStream_t s)
{
    hipLaunchKernelGGL(ppfs::flag_kernel, dim3(1), dim3(64), 0, s, flag, v);
    return hipGetLastError();
}

// src holds src_rows rows; idx[i] < src_rows
extern "C" hipError_t ppfs_gather_rows_launch(const uint8_t* src, uint64_t src_rows, uint8_t* dst, const uint32_t* idx,
    uint32_t nrows, uint32_t row_bytes, hipStream_t s)
{
    if (nrows == 0)
        return hipSuccess;
    const uint32_t grid = nrows < 4096u ? nrows : 4096u;
    hipLaunchKernelGGL(ppfs::gather_rows_kernel, dim3(grid), dim3(256), 0, s, src, src_rows, dst, idx, nrows, row_bytes);
    return hipGetLastError();
}

// ---- block lists (list_path.cpp): image rows <-> a dense staging copy ----
// A list call names nb rows of an image of image_blocks rows of `raw` bytes, in any order: entry i is
// image row index[i].  With raw = 255 (every RS case) an image row has every byte alignment and a
// staging row has another, so neither kernel can copy 16-byte pieces from equal offsets as
// gather_rows_kernel does.  Both work in 16-byte windows ALIGNED ON THE SIDE THEY STORE TO, read the
// other side as the aligned dwords that cover the window (five, or four when the two sides happen to
// agree mod 4) and bring them into place with v_alignbyte; only the windows that hold a row's head
// or tail fall back to bytes.  Positions are 32-bit: the launchers refuse nb * raw >= 2^32.
namespace ppfs {

// load16_funnel: funnel.hpp

// stage row i = image row index[i] for i < nb; an entry with index[i] >= image_blocks is never
// dereferenced and its row becomes zeros.  One lane per 16-byte window of the staging copy
// (16-byte aligned, capacity nb * raw rounded up to 16: the last window is stored whole, its excess
// zero).  A window inside one row takes the aligned-dword path unless those dwords would reach
// outside the image (only next to the image's two ends); a window over a row boundary is put
// together from byte loads.  Every store is one aligned 16 bytes.
__global__ __launch_bounds__(256) void gather_blocks_kernel(const uint8_t* __restrict__ img, uint64_t image_blocks,
    const uint32_t* __restrict__ index, uint32_t nb, uint32_t raw, uint8_t* __restrict__ stage)
{
    const uint32_t total = nb * raw, nwin = (total + 15u) / 16u;
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nwin)
        return;
    const uint8_t* img_end = img + image_blocks * raw;
    const uint32_t P = 16u * c;
    uint32_t row = P / raw, col = P - row * raw;
    uint32_t idx = PPFS_DBG_OK(index + row, 4, index, (uint64_t)nb * 4) ? index[row] : 0xFFFFFFFFu;
    uint4 v = make_uint4(0, 0, 0, 0);
    bool done = false;
    if (col + 16u <= raw) {
        if (idx >= image_blocks) {
            done = true;
        } else {
            const uint8_t* p = img + (uint64_t)idx * raw + col;
            const uint8_t* a = (const uint8_t*)((uintptr_t)p & ~(uintptr_t)3);
            const uint32_t span = ((uintptr_t)p & 3u) ? 20u : 16u;
            if (a >= img && a + span <= img_end && PPFS_DBG_OK(a, span, img, image_blocks * raw)) {
                v = load16_funnel(p);
                done = true;
            }
        }
    }
    if (!done) {
        uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
            uint32_t b = 0;
            if (row < nb && idx < image_blocks) {
                const uint8_t* p = img + (uint64_t)idx * raw + col;
                if (PPFS_DBG_OK(p, 1, img, image_blocks * raw))
                    b = *p;
            }
            w[j >> 2] |= b << (8u * (j & 3u));
            if (++col == raw) {
                col = 0;
                ++row;
                idx = row < nb && PPFS_DBG_OK(index + row, 4, index, (uint64_t)nb * 4) ? index[row] : 0xFFFFFFFFu;
            }
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (PPFS_DBG_OK(stage + P, 16, stage, (uint64_t)nwin * 16))
        *(uint4*)(stage + P) = v;
}

// image row index[i] = stage row i for the entries that are in range and that `mode` selects:
// 0 every entry, 1 status[i] == 1 (a decode's write-back), 2 status[i] != 5 (a write whose old
// block passed its check).  Row i's destination is cut into the 16-byte ALIGNED windows of the image
// that it touches (at most K = (raw + 15) / 16 + 1), one lane each: a window wholly inside the row
// is one aligned 16-byte store of funnel-shifted staging dwords, the head and tail windows store
// their bytes of the row one by one.  So every destination byte has exactly one writer, nothing
// outside a selected row is written and nothing of the image is read.  The staging copy is read
// as aligned dwords up to its capacity (nb * raw rounded up to 16).
__global__ __launch_bounds__(256) void scatter_blocks_kernel(const uint8_t* __restrict__ stage, uint8_t* __restrict__ img,
    uint64_t image_blocks, const uint32_t* __restrict__ index, const uint8_t* __restrict__ status, int mode, uint32_t nb,
    uint32_t raw, uint32_t K)
{
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (uint64_t)nb * K)
        return;
    const uint32_t i = (uint32_t)(item / K), k = (uint32_t)(item - (uint64_t)i * K);
    if (!PPFS_DBG_OK(index + i, 4, index, (uint64_t)nb * 4))
        return;
    const uint32_t idx = index[i];
    if (idx >= image_blocks)
        return;
    if (mode != 0) {
        if (!PPFS_DBG_OK(status + i, 1, status, nb))
            return;
        const uint32_t st = status[i];
        if (mode == 1 ? st != 1u : st == 5u)
            return;
    }
    uint8_t* d = img + (uint64_t)idx * raw;
    const uint8_t* s = stage + (uint64_t)i * raw;
    const uintptr_t win = ((uintptr_t)d & ~(uintptr_t)15) + 16u * (uintptr_t)k;
    const uintptr_t lo = win > (uintptr_t)d ? win : (uintptr_t)d;
    const uintptr_t hi = win + 16u < (uintptr_t)d + raw ? win + 16u : (uintptr_t)d + raw;
    if (lo >= hi)
        return;
    const uint32_t off = (uint32_t)(lo - (uintptr_t)d), len = (uint32_t)(hi - lo);
    if (!PPFS_DBG_OK(d + off, len, img, image_blocks * raw)
        || !PPFS_DBG_OK(s + off, len, stage, (((uint64_t)nb * raw + 15u) / 16u) * 16u))
        return;
    if (len == 16u) {
        *(uint4*)(d + off) = load16_funnel(s + off);
    } else {
        for (uint32_t b = 0; b < len; ++b)
            d[off + b] = s[off + b];
    }
}

// the out-of-range entries of a list: status PPFS_ECC_OUT_OF_BOUNDS (9) and a zero payload, after
// the codec ran over their zero staging rows.  One thread per entry; such entries are a caller's
// mistake, not a path to tune.
__global__ __launch_bounds__(256) void list_oob_kernel(const uint32_t* __restrict__ index, uint32_t nb, uint64_t image_blocks,
    uint8_t* __restrict__ status, uint8_t* __restrict__ data, uint32_t data_bytes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || !PPFS_DBG_OK(index + i, 4, index, (uint64_t)nb * 4) || index[i] < image_blocks)
        return;
    if (status && PPFS_DBG_OK(status + i, 1, status, nb))
        status[i] = 9;
    if (data && PPFS_DBG_OK(data + (uint64_t)i * data_bytes, data_bytes, data, (uint64_t)nb * data_bytes))
        for (uint32_t b = 0; b < data_bytes; ++b)
            data[(uint64_t)i * data_bytes + b] = 0;
}

// ---- byte extents (extent_path.cpp): payload staging <-> the caller's packed buffer ----
// Entry i of a piece names len = min(length, ds - offset) bytes of payload i of the staging P (stride
// ds) and the same number at buf + pos.  An entry is valid when its block is in the image, its offset
// is at most ds and [pos, pos + len) lies inside the buf_bytes of the caller's buffer.

// index[i] = valid ? block : 0xFFFFFFFF, the index the gather, scatter and range-mark kernels above
// and the copy kernel below go by.  One thread per entry.  image_blocks <= 0xFFFFFFFF (the launcher).
__global__ __launch_bounds__(256) void extent_index_kernel(const ppfs_ecc_extent* __restrict__ ext, uint32_t nb,
    uint64_t image_blocks, uint32_t ds, uint64_t buf_bytes, uint32_t* __restrict__ index)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || !PPFS_DBG_OK(ext + i, 16, ext, (uint64_t)nb * 16) || !PPFS_DBG_OK(index + i, 4, index, (uint64_t)nb * 4))
        return;
    const ppfs_ecc_extent e = ext[i];
    bool ok = e.block < image_blocks && e.offset <= ds;
    if (ok) {
        const uint32_t room = ds - e.offset, len = e.length < room ? e.length : room;
        ok = e.pos <= buf_bytes && len <= buf_bytes - e.pos;
    }
    index[i] = ok ? e.block : 0xFFFFFFFFu;
}

// TO_STAGE = false (pack, a read): buf[pos, pos + len) = P[i*ds + offset ...), zeros where status[i] is 5.
// TO_STAGE = true (overlay, a write): P[i*ds + offset ...) = buf[pos, pos + len).
// Neither side is aligned and the two are aligned differently.  The scatter kernel's shape: entry i's
// destination is cut into the 16-byte ALIGNED windows it touches (at most K = (ds + 15) / 16 + 1), one
// lane each; a window wholly inside the segment is one aligned 16-byte store of funnel-shifted source
// dwords, the head and tail windows store their own bytes one by one.  So every destination byte has
// exactly one writer and nothing outside [dst, dst + len) is written.  The funnel reads the aligned
// dwords that cover its 16 bytes: where those would reach outside the source ([src_lo, src_hi): the
// caller's buffer in the overlay direction, the staging's capacity in the pack direction) the window
// takes the byte path, as the gather does next to the image's ends.  Entries staged as 0xFFFFFFFF are
// skipped; the validity of the others (extent_index_kernel) bounds every address formed here.
template <bool TO_STAGE>
__global__ __launch_bounds__(256) void extent_copy_kernel(const ppfs_ecc_extent* __restrict__ ext,
    const uint32_t* __restrict__ index, const uint8_t* __restrict__ status, uint32_t nb, uint32_t ds, uint32_t K,
    uint8_t* stage, uint64_t stage_cap, uint8_t* buf, uint64_t buf_bytes)
{
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (uint64_t)nb * K)
        return;
    const uint32_t i = (uint32_t)(item / K), k = (uint32_t)(item - (uint64_t)i * K);
    if (!PPFS_DBG_OK(index + i, 4, index, (uint64_t)nb * 4) || index[i] == 0xFFFFFFFFu
        || !PPFS_DBG_OK(ext + i, 16, ext, (uint64_t)nb * 16))
        return;
    const ppfs_ecc_extent e = ext[i];
    if (e.offset >= ds)
        return;
    const uint32_t room = ds - e.offset, seg = e.length < room ? e.length : room;
    uint8_t* in_stage = stage + (uint64_t)i * ds + e.offset;
    uint8_t* in_buf = buf + e.pos;
    uint8_t* d = TO_STAGE ? in_stage : in_buf;
    const uint8_t* s = TO_STAGE ? in_buf : in_stage;
    const uintptr_t win = ((uintptr_t)d & ~(uintptr_t)15) + 16u * (uintptr_t)k;
    const uintptr_t lo = win > (uintptr_t)d ? win : (uintptr_t)d;
    const uintptr_t hi = win + 16u < (uintptr_t)d + seg ? win + 16u : (uintptr_t)d + seg;
    if (lo >= hi)
        return;
    const uint32_t off = (uint32_t)(lo - (uintptr_t)d), len = (uint32_t)(hi - lo);
    if (!PPFS_DBG_OK(in_stage + off, len, stage, stage_cap) || !PPFS_DBG_OK(in_buf + off, len, buf, buf_bytes))
        return;
    bool zero = false;
    if (!TO_STAGE && status && PPFS_DBG_OK(status + i, 1, status, nb))
        zero = status[i] == 5u;
    const uint8_t* src_lo = TO_STAGE ? buf : stage;
    const uint8_t* src_hi = TO_STAGE ? buf + buf_bytes : stage + stage_cap;
    if (len == 16u) {
        if (zero) {
            *(uint4*)(d + off) = make_uint4(0, 0, 0, 0);
            return;
        }
        const uint8_t* p = s + off;
        const uint8_t* a = (const uint8_t*)((uintptr_t)p & ~(uintptr_t)3);
        const uint32_t span = ((uintptr_t)p & 3u) ? 20u : 16u;
        if (a >= src_lo && a + span <= src_hi) {
            *(uint4*)(d + off) = load16_funnel(p);
            return;
        }
    }
    for (uint32_t b = 0; b < len; ++b)
        d[off + b] = zero ? (uint8_t)0 : s[off + b];
}
} // namespace ppfs

// stage: 16-byte aligned, capacity nb * raw rounded up to 16
extern "C" hipError_t ppfs_gather_blocks_launch(const uint8_t* img, uint64_t image_blocks, const uint32_t* index, uint32_t nb,
    uint32_t raw, uint8_t* stage, hipStream_t s)
{
    if (nb == 0 || raw == 0)
        return hipSuccess;
    if ((uint64_t)nb * raw >= (1ull << 32) || ((uintptr_t)stage & 15u))
        return hipErrorInvalidValue;
    const uint32_t nwin = (nb * raw + 15u) / 16u;
    hipLaunchKernelGGL(ppfs::gather_blocks_kernel, dim3((nwin + 255u) / 256u), dim3(256), 0, s, img, image_blocks, index, nb,
        raw, stage);
    return hipGetLastError();
}

// mode: 0 every in-range entry, 1 those with status 1, 2 those with status other than 5
extern "C" hipError_t ppfs_scatter_blocks_launch(const uint8_t* stage, uint8_t* img, uint64_t image_blocks,
    const uint32_t* index, const uint8_t* status, int mode, uint32_t nb, uint32_t raw, hipStream_t s)
{
    if (nb == 0 || raw == 0)
        return hipSuccess;
    if ((uint64_t)nb * raw >= (1ull << 32) || ((uintptr_t)stage & 15u) || mode < 0 || mode > 2 || (mode && !status))
        return hipErrorInvalidValue;
    const uint32_t K = (raw + 15u) / 16u + 1u;
    const uint64_t grid = ((uint64_t)nb * K + 255u) / 256u;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ppfs::scatter_blocks_kernel, dim3((uint32_t)grid), dim3(256), 0, s, stage, img, image_blocks, index,
        status, mode, nb, raw, K);
    return hipGetLastError();
}

extern "C" hipError_t ppfs_list_oob_launch(const uint32_t* index, uint32_t nb, uint64_t image_blocks, uint8_t* status,
    uint8_t* data, uint32_t data_bytes, hipStream_t s)
{
    if (nb == 0 || (!status && !(data && data_bytes)))
        return hipSuccess;
    hipLaunchKernelGGL(ppfs::list_oob_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, s, index, nb, image_blocks, status,
        data_bytes ? data : nullptr, data_bytes);
    return hipGetLastError();
}

// ext: 8-byte aligned; image_blocks <= 0xFFFFFFFF, so that 0xFFFFFFFF names no block
extern "C" hipError_t ppfs_extent_index_launch(const ppfs_ecc_extent* ext, uint32_t nb, uint64_t image_blocks, uint32_t ds,
    uint64_t buf_bytes, uint32_t* index, hipStream_t s)
{
    if (nb == 0)
        return hipSuccess;
    if (((uintptr_t)ext & 7u) || ((uintptr_t)index & 3u) || image_blocks > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ppfs::extent_index_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, s, ext, nb, image_blocks, ds,
        buf_bytes, index);
    return hipGetLastError();
}

// to_stage 0: pack (buf is written, status may be null), 1: overlay (buf is only read).  stage: 16-byte
// aligned payloads at stride ds with a capacity of stage_cap >= nb * ds bytes, a multiple of 16.
extern "C" hipError_t ppfs_extent_copy_launch(int to_stage, const ppfs_ecc_extent* ext, const uint32_t* index,
    const uint8_t* status, uint32_t nb, uint32_t ds, uint8_t* stage, uint64_t stage_cap, uint8_t* buf, uint64_t buf_bytes,
    hipStream_t s)
{
    if (nb == 0 || ds == 0 || buf_bytes == 0)
        return hipSuccess;
    if (((uintptr_t)ext & 7u) || ((uintptr_t)stage & 15u) || (stage_cap & 15u) || (uint64_t)nb * ds > stage_cap || !buf)
        return hipErrorInvalidValue;
    const uint32_t K = (ds + 15u) / 16u + 1u;
    const uint64_t grid = ((uint64_t)nb * K + 255u) / 256u;
    if (grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    if (to_stage)
        hipLaunchKernelGGL(ppfs::extent_copy_kernel<true>, dim3((uint32_t)grid), dim3(256), 0, s, ext, index, status, nb, ds, K,
            stage, stage_cap, buf, buf_bytes);
    else
        hipLaunchKernelGGL(ppfs::extent_copy_kernel<false>, dim3((uint32_t)grid), dim3(256), 0, s, ext, index, status, nb, ds, K,
            stage, stage_cap, buf, buf_bytes);
    return hipGetLastError();
}

PPFS_DBG_ACCESSOR(ppfs_dbg_faults_vote)

// Positive control of the PPFS_ECC_DEBUG checks (tests/test_gpu_hygiene.py): a gather of row 5
// from a 4-row source must be reported and skipped.  Returns the number of reports (the counter is
// restored afterwards, so the suite's per-test accounting is unaffected); -1 in normal builds.
#ifdef PPFS_ECC_DEBUG
extern "C" long long ppfs_ecc_debug_selftest(void)
{
    uint8_t *src = nullptr, *dst = nullptr;
    uint32_t* idx = nullptr;
    const uint32_t bad = 5;
    unsigned long long before = 0, after = 0;
    long long r = -2;
    if (hipMalloc(&src, 4 * 16) == hipSuccess && hipMalloc(&dst, 16) == hipSuccess && hipMalloc(&idx, 4) == hipSuccess
        && hipMemcpy(idx, &bad, 4, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpyFromSymbol(&before, HIP_SYMBOL(ppfs::dbg::g_faults), sizeof(before)) == hipSuccess
        && ppfs_gather_rows_launch(src, 4, dst, idx, 1, 16, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess
        && hipMemcpyFromSymbol(&after, HIP_SYMBOL(ppfs::dbg::g_faults), sizeof(after)) == hipSuccess
        && hipMemcpyToSymbol(HIP_SYMBOL(ppfs::dbg::g_faults), &before, sizeof(before)) == hipSuccess)
        r = (long long)(after - before);
    (void)hipFree(src);
    (void)hipFree(dst);
    (void)hipFree(idx);
    return r;
}
#else
extern "C" long long ppfs_ecc_debug_selftest(void) { return -1; }
#endif
