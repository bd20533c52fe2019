#pragma once
// rs_wg_list.hpp -- the block-list decode of RS(255, 255-2t), 2t <= 8, in one kernel: entry i of the
// list is image row index[i], fetched straight from the image into the LDS tile.  No staging copy, no
// scatter, no range-mark pass (list_path.cpp's staged pipeline, which every other codec keeps).
//
// The static-walk decode of rs_wg.hpp with another loader: the LDS tile has the contiguous kernel's
// layout (64 rows packed at 255 B behind PAD), so the remainder, correction and emission phases
// are that kernel's, unchanged (rs_wg.hpp's tile phases; this file holds the loader and the walk);
// the correction takes the image as its write-back target and
// index[i] as its block, so corrected bytes go in place at image + index[i] * 255 + pos, and
// payloads and statuses come out in list order.
//
// Loader.  LDS-DMA cannot serve: a listed row starts at any byte of the image.  Each thread owns 4 of
// the tile's 1,020 16-byte windows (as dma_tile does) and reads each by the plan of list_fetch.hpp:
// the aligned dwords covering the window's bytes of one row, funnel-shifted (funnel.hpp); two such
// reads merged by a byte mask for the 60 windows that hold a row boundary; single bytes where those
// dwords would leave the image (next to its two ends only).  The next tile's windows are
// read into registers (4 x uint4) after barrier A and stored into the other tile buffer after this
// tile's emission reads.  The tile's 64 indices are one coalesced load of wave 1 and wait in a
// 256-byte LDS slot from one tile earlier, so a window's address depends on no global load of the
// same iteration.  The compiler places the vmcnt waits (these are ordinary register loads).
//
// An entry index[i] >= image_blocks (0xFFFFFFFF among them) is never dereferenced: its LDS row is
// zeros -- a valid codeword, so the payload comes out zero by itself -- wave 0 stores status 9
// (PPFS_ECC_OUT_OF_BOUNDS) for it, and it takes no write-back.
//
// The block-list encode (rs_wg_encode_list_kernel, at the end of the file) is the other direction:
// the static-walk encode with another emission, which stores codeword i at image + index[i] * 255
// by the store plan of list_store.hpp.
#include "funnel.hpp"
#include "list_fetch.hpp"
#include "list_store.hpp"
#include "rs_wg.hpp"

namespace ppfs {
namespace wg {

__device__ __forceinline__ uint4 and4(uint4 a, bool keep)
{
    const uint32_t m = keep ? ~0u : 0u;
    return make_uint4(a.x & m, a.y & m, a.z & m, a.w & m);
}

// window w of the tile, or window 0 for the 4 slots past the tile's 1,020 (k = 3, tid >= 252), which
// are fetched like any other and never stored
__device__ __forceinline__ uint32_t list_window(uint32_t tid, int k)
{
    const uint32_t w = tid + 256u * k;
    return k < 3 || w < listfetch::TILE_WINDOWS ? w : 0u;
}

// The thread's 4 windows of the tile whose 64 entries are slot[0..63] (window tid + 256 k), into
// registers.  Straight-line on purpose: the plans of all 8 parts (a window's piece of its row, and of
// the next row where it holds a boundary), then all the loads, then the shifts and merges, so one
// round trip to memory serves the whole tile.  A part that is not read through the funnel (no block,
// an interior window's second part, a BYTES part) loads from `safe` instead, the engine's own tables,
// and the result is dropped.  Returns the windows that hold a BYTES part (bit k): those are not taken
// from v[k] but written byte by byte by list_fetch_slow.
__device__ __forceinline__ uint32_t list_fetch_tile(uint4 (&v)[4], const uint8_t* img, uint64_t image_blocks,
    const uint32_t* slot, uint32_t tid, const uint8_t* safe)
{
    const uint64_t base = (uint64_t)(uintptr_t)img;
    [[maybe_unused]] const uint64_t img_bytes = image_blocks * listfetch::ROW;
    uint32_t n0[4], sa[4], sb[4], slow = 0;
    Funnel5 ra[4], rb[4];
    bool fa[4], fb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const listfetch::Window x = listfetch::window_of(list_window(tid, k));
        const listfetch::Part pa = listfetch::part_a(base, image_blocks, x, slot[x.row]);
        const listfetch::Part pb = listfetch::part_b(base, image_blocks, x, slot[x.row + (x.n0 < 16u ? 1u : 0u)]);
        // addresses formed from the image pointer, so the loads are global loads
        const uint8_t* aa = img + (pa.a - base);
        const uint8_t* ab = img + (pb.a - base);
        fa[k] = pa.kind == listfetch::FUNNEL && PPFS_DBG_OK(aa, pa.span, img, img_bytes);
        fb[k] = pb.kind == listfetch::FUNNEL && PPFS_DBG_OK(ab, pb.span, img, img_bytes);
        ra[k] = funnel_load5((const uint32_t*)(fa[k] ? aa : safe));
        rb[k] = funnel_load5((const uint32_t*)(fb[k] ? ab : safe));
        n0[k] = x.n0;
        sa[k] = (uint32_t)pa.p0 & 3u;
        sb[k] = (uint32_t)pb.p0 & 3u;
        if (pa.kind == listfetch::BYTES || pb.kind == listfetch::BYTES)
            slow |= 1u << k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 a = and4(funnel_shift(ra[k], sa[k]), fa[k]);
        const uint4 b = and4(funnel_shift(rb[k], sb[k]), fb[k]);
        const M128 m = range_mask(0, n0[k]);
        v[k] = make_uint4(bfi((uint32_t)m.lo, a.x, b.x), bfi((uint32_t)(m.lo >> 32), a.y, b.y), bfi((uint32_t)m.hi, a.z, b.z),
            bfi((uint32_t)(m.hi >> 32), a.w, b.w));
    }
    return slow;
}

// The windows of `slow` (next to the image's two ends only), byte by byte into the tile buffer at
// dst: the byte loop of gather_blocks_kernel.  Rolled loops: a rare path that must cost the common
// one no registers.  (img, img_bytes): the image, for the PPFS_ECC_DEBUG bounds checks.
__device__ __forceinline__ void list_fetch_slow(uint8_t* dst, const uint8_t* img, uint64_t image_blocks, const uint32_t* slot,
    uint32_t tid, uint32_t slow)
{
    const uint64_t base = (uint64_t)(uintptr_t)img;
    [[maybe_unused]] const uint64_t img_bytes = image_blocks * listfetch::ROW;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = tid + 256u * k;
        if (!((slow >> k) & 1u) || w >= listfetch::TILE_WINDOWS)
            continue;
        const listfetch::Window x = listfetch::window_of(w);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && x.n0 == 16u)
                break;
            const listfetch::Part p = h == 0 ? listfetch::part_a(base, image_blocks, x, slot[x.row])
                                             : listfetch::part_b(base, image_blocks, x, slot[x.row + 1u]);
            const uint8_t* s = img + (p.p0 - base);
#pragma unroll 1
            for (uint32_t j = p.lo; j < p.hi; ++j) {
                uint8_t b = 0;
                if (p.kind != listfetch::SKIP && PPFS_DBG_OK(s + j, 1, img, img_bytes))
                    b = s[j];
                dst[16u * w + j] = b;
            }
        }
    }
}

__device__ __forceinline__ void list_store_tile(uint8_t* dst, const uint4 (&v)[4], uint32_t tid, uint32_t slow)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = tid + 256u * k;
        if ((k < 3 || w < listfetch::TILE_WINDOWS) && !((slow >> k) & 1u))
            *(uint4*)(dst + 16u * w) = v[k];
    }
}

// entry i of the list; past its end: no block
__device__ __forceinline__ uint32_t list_entry(const uint32_t* __restrict__ index, uint64_t i, uint64_t nblocks)
{
    return i < nblocks && PPFS_DBG_OK(index + i, 4, index, nblocks * 4u) ? index[i] : 0xFFFFFFFFu;
}

template <int T2, int WPC = 3, int NTST = 1>
__global__ __launch_bounds__(256, WPC) void rs_wg_decode_list_kernel(uint8_t* image, uint64_t image_blocks,
    const uint32_t* __restrict__ index, uint8_t* __restrict__ data, uint8_t* __restrict__ status, uint64_t nblocks,
    const uint8_t* __restrict__ tables, int write_back)
{
    using L = RsWgLayout<T2>;
    using D = Lds<T2, true, 2>;
    constexpr int OFF_IDX = D::BYTES; // the next tile's 64 entries
    constexpr int LDS_ALLOC = lds_alloc<D::BYTES + 256, WPC>();
    static_assert(WPC * LDS_ALLOC <= 163840, "LDS for WPC workgroups per CU");
    static_assert(OFF_IDX % 16 == 0, "aligned index slot");
    constexpr int K = L::K;
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_ALLOC];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = wave_id();
    const uint32_t row = lane_row(lane);
    const bool wb = write_back != 0, want = data != nullptr;
    const uint64_t img_bytes = image_blocks * 255u;
    uint32_t* const slot = (uint32_t*)(lds + OFF_IDX);
    tables_to_lds<D::TBL, D::OFF_PAR>(lds, tables, tid);
    const uint64_t nfull = nblocks / TB, ntiles = (nblocks + TB - 1) / TB;
    const uint64_t G = gridDim.x;
    // One loop for every tile of this workgroup, the partial last tile of the list included: an
    // iteration fetches tile f into registers and runs the phases on tile t = f - G, fetched by the
    // iteration before (the first iteration only fetches; the last only computes).
    uint64_t t = 0, f = blockIdx.x;
    if (f >= ntiles)
        return;
    bool first = true;
    uint32_t cur = 1, pc = 0;
    uint32_t my_idx = 0xFFFFFFFFu; // wave 0: the entry of this lane's row of tile t
    if (wave == 1)
        slot[lane] = list_entry(index, f * TB + lane, nblocks);
    for (;;) {
        barrier_lds(); // A: tile t in LDS, the slot holds tile f's entries, last tile's emission reads done
        const uint32_t buf = D::OFF_BUF + cur * BUF, par = D::OFF_PAR + pc * 512u;
        const bool have = f < ntiles, far = f + G < ntiles;
        uint4 v[4];
        uint32_t next_idx = 0xFFFFFFFFu, far_idx = 0xFFFFFFFFu, slow = 0;
        uint8_t* const nbuf = lds + D::OFF_BUF + (cur ^ 1u) * BUF + PAD; // held tile t - G: free since barrier A
        if (have) {
            // the windows' row / column / mask arithmetic is redone every tile (a few ALU operations):
            // hoisted out of the loop it would hold some 30 registers through the correction phase
            uint32_t ftid = tid;
            asm volatile("" : "+v"(ftid));
            slow = list_fetch_tile(v, image, image_blocks, slot, ftid, tables);
            if (slow)
                list_fetch_slow(nbuf, image, image_blocks, slot, ftid, slow);
            if (wave == 0)
                next_idx = slot[row];
        }
        if (wave == 1 && far)
            far_idx = list_entry(index, (f + G) * TB + lane, nblocks);
        if (!first) {
            if (wave == 0)
                *(uint64_t*)(lds + D::OFF_PAR + (pc ^ 1u) * 512u + 8u * lane) = 0;
            phase_remainder<T2, 255>(lds, buf, par, wave, row);
        }
        barrier_lds(); // B: remainders complete; every read of the slot done
        if (wave == 1 && far)
            slot[lane] = far_idx;
        // entries of tile t: 64, or the list's last nblocks % 64 (their rows past the list's end are
        // zeros, entries that name no block)
        const uint32_t nb = t < nfull ? (uint32_t)TB : (uint32_t)(nblocks - t * TB);
        if (!first && wave == 0) {
            const bool listed = row < nb, valid = listed && my_idx < image_blocks;
            const uint32_t st = phase_correct<T2>(lds, buf, par, row, valid, image, my_idx, wb, img_bytes);
            if (status && listed && PPFS_DBG_OK(status + t * TB + row, 1, status, nblocks))
                status[t * TB + row] = valid ? (uint8_t)st : (uint8_t)9;
        }
        barrier_lds(); // C: corrections patched into the LDS rows
        if (!first && want) {
            uint8_t* dst = data + t * (TB * K);
            if (nb == (uint32_t)TB)
                dec_emit_tile<T2, NTST>(lds, buf, dst, tid, data, nblocks * K);
            else
                dec_emit_partial<T2>(lds, buf, dst, nb * (uint32_t)K, tid, data, nblocks * K);
        }
        if (!have)
            break;
        list_store_tile(nbuf, v, tid, slow);
        my_idx = next_idx;
        t = f;
        f += G;
        cur ^= 1u;
        pc ^= 1u;
        first = false;
    }
}

// ------------------------------------------------------------------------------------
// The block-list encode: payload i of the (contiguous, list-order) payload array becomes the
// codeword at image + index[i] * 255.  The static-walk encode of rs_wg.hpp with another emission:
// loader (LDS-DMA of the packed payload rows), remainder phase and parity slots are that kernel's;
// the emission cuts each LDS row by the store plan of list_store.hpp instead of cutting the packed
// codeword tile into 16-byte pieces, and takes each piece from enc_piece_at, the contiguous
// emission's own assembly at any byte of a row.  No staging rows, no scatter.
//
// Buffering: two tile buffers, the next tile's DMA issued after barrier A.  The waves' store counts
// differ here (a wave's round has 60 or 64 lanes on full windows, one wave has the edges, rows that
// name no block store nothing), so the contiguous encode's counted wait -- "4 stores per wave per
// tile" -- does not hold, and no count is kept: every wave waits vmcnt(0) once per tile, after its
// remainder phase and before barrier B.  What is outstanding there is the last tile's stores and
// this iteration's DMA, both issued a whole remainder phase earlier; this tile's stores are issued
// after it and fly through the next tile's remainder phase.  Exact because it counts nothing: after
// barrier B every wave's DMA pieces of the next tile have landed, which is all barrier A of the next
// iteration needs.
//
// The tile's 64 entries are one coalesced load of wave 1, issued at the top of the iteration before
// and parked in one of two 256-byte LDS slots after that iteration's vmcnt(0), so a store address
// depends on no global load of its own iteration.  The partial last tile is staged by plain loads
// (never past data + nblocks * K) and goes through the same emission: list_entry gives the rows past
// the list's end the entry 0xFFFFFFFF, which stores nothing.
// ------------------------------------------------------------------------------------
template <int NT, typename T> __device__ __forceinline__ void st_narrow(uint8_t* dst, T v)
{
    if constexpr (NT)
        __builtin_nontemporal_store(v, (T*)dst);
    else
        *(T*)dst = v;
}

// bytes [o, o + 8) of the 16-byte piece v (o in [0, 16); bytes past the piece read as zero)
__device__ __forceinline__ uint64_t piece_bytes8(uint4 v, uint32_t o)
{
    const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
    const uint64_t a = o < 8u ? lo : hi, b = o < 8u ? hi : 0ull;
    const uint32_t s = 8u * (o & 7u);
    return s ? (a >> s) | (b << (64u - s)) : a;
}

// Emission of the tile in `buf` (parity slots `par`) whose 64 entries are slot[0..63]: this thread's 4
// slots of the store plan (slot tid + 256 k)
template <int T2, int NTST>
__device__ __forceinline__ void list_emit_tile(const uint8_t* lds, uint32_t buf, uint32_t par, const uint32_t* slot,
    uint8_t* image, uint64_t image_blocks, uint32_t tid)
{
    const uint64_t base = (uint64_t)(uintptr_t)image;
    [[maybe_unused]] const uint64_t img_bytes = image_blocks * liststore::ROW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = tid + 256u * k;
        if (k < 3 || s < liststore::TILE_FULL) { // k = 3: waves 0..2
            const liststore::Full f = liststore::full_slot(s);
            const liststore::Dst x = liststore::row_dst(base, image_blocks, slot[f.row]);
            const liststore::Piece pc = liststore::full_piece(x, f.j);
            const uint4 v = enc_piece_at<T2>(lds, buf, par, f.row, pc.c0);
            if (x.live) {
                uint8_t* p = image + (pc.a - base);
                if (PPFS_DBG_OK(p, 16, image, img_bytes))
                    st_nt<NTST>(p, v);
            }
        } else { // the 64 edges: wave 3, a row per lane
            const uint32_t r = s - liststore::TILE_FULL;
            const liststore::Dst x = liststore::row_dst(base, image_blocks, slot[r]);
            const uint32_t tail0 = x.h + liststore::TAIL_C0;
            const uint4 hv = enc_piece_at<T2>(lds, buf, par, r, 0u), tv = enc_piece_at<T2>(lds, buf, par, r, tail0);
#pragma unroll
            for (int q = 0; q < (int)liststore::EDGE_PIECES; ++q) {
                const liststore::Piece pc = liststore::edge_piece(x, (uint32_t)q);
                const uint64_t bits = piece_bytes8(q < 4 ? hv : tv, pc.c0 - (q < 4 ? 0u : tail0));
                if (x.live && pc.size) {
                    uint8_t* p = image + (pc.a - base);
                    if (!PPFS_DBG_OK(p, pc.size, image, img_bytes))
                        continue;
                    const int SIZE = q < 4 ? 1 << q : 8 >> (q - 4); // pc.size where there is a piece; a constant once unrolled
                    if (SIZE == 1)
                        st_narrow<NTST>(p, (uint8_t)bits);
                    else if (SIZE == 2)
                        st_narrow<NTST>(p, (uint16_t)bits);
                    else if (SIZE == 4)
                        st_narrow<NTST>(p, (uint32_t)bits);
                    else
                        st_narrow<NTST>(p, bits);
                }
            }
        }
    }
}

template <int T2, int WPC = 3, int NTST = 1>
__global__ __launch_bounds__(256, WPC) void rs_wg_encode_list_kernel(const uint8_t* __restrict__ data, uint8_t* image,
    uint64_t image_blocks, const uint32_t* __restrict__ index, uint64_t nblocks, const uint8_t* __restrict__ tables)
{
    using L = RsWgLayout<T2>;
    using D = Lds<T2, false, 2>;
    constexpr int OFF_IDX = D::BYTES; // two sets of 64 entries: this tile's and the next one's
    constexpr int LDS_ALLOC = lds_alloc<D::BYTES + 512, WPC>();
    static_assert(WPC * LDS_ALLOC <= 163840, "LDS for WPC workgroups per CU");
    static_assert(OFF_IDX % 16 == 0, "aligned index slots");
    constexpr int K = L::K;
    constexpr int IN_PIECES = TB * K / 16;
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_ALLOC];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = wave_id();
    const uint32_t row = lane_row(lane);
    uint32_t* const slot = (uint32_t*)(lds + OFF_IDX);
    tables_to_lds<D::TBL, D::OFF_PAR>(lds, tables, tid);
    const uint64_t nfull = nblocks / TB, ntiles = (nblocks + TB - 1) / TB;
    const uint64_t G = gridDim.x;
    uint64_t t = blockIdx.x;
    if (t >= ntiles)
        return;
    uint32_t cur = 0, pc = 0; // tile buffer; parity-slot and entry set
    if (t < nfull)
        dma_tile<IN_PIECES>(lds + D::OFF_BUF + PAD, data + t * (TB * K), tid, data, nblocks * K);
    if (wave == 1)
        slot[lane] = list_entry(index, t * TB + lane, nblocks);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (; t < ntiles; t += G) {
        barrier_lds(); // A: tile t and its entries in LDS, last tile's emission reads done
        const uint32_t buf = D::OFF_BUF + cur * BUF, par = D::OFF_PAR + pc * 512u;
        const uint64_t nx = t + G;
        if (nx < nfull)
            dma_tile<IN_PIECES>(lds + D::OFF_BUF + (cur ^ 1u) * BUF + PAD, data + nx * (TB * K), tid, data, nblocks * K);
        uint32_t next_idx = 0xFFFFFFFFu;
        if (wave == 1 && nx < ntiles)
            next_idx = list_entry(index, nx * TB + lane, nblocks);
        if (t >= nfull) { // the partial last tile: no DMA brought it
            const uint32_t nb = (uint32_t)(nblocks - t * TB);
            if (PPFS_DBG_OK(data + t * (TB * K), nb * K, data, nblocks * K))
                stage_bytes(lds + buf + PAD, data + t * (TB * K), nb * K, tid);
            barrier_lds();
        }
        if (wave == 0)
            *(uint64_t*)(lds + D::OFF_PAR + (pc ^ 1u) * 512u + 8u * lane) = 0;
        phase_remainder<T2, K, D::NMAP>(lds, buf, par, wave, row);
        // the last tile's stores and the next tile's DMA and entries (see the header comment)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 1 && nx < ntiles)
            slot[64u * (pc ^ 1u) + lane] = next_idx;
        barrier_lds(); // B: parity slots complete, the next tile landed
        list_emit_tile<T2, NTST>(lds, buf, par, slot + 64u * pc, image, image_blocks, tid);
        cur ^= 1u;
        pc ^= 1u;
    }
}

} // namespace wg
} // namespace ppfs
