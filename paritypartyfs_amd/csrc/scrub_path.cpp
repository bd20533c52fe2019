// scrub_path.cpp -- the scrubs of the ppfs_ecc C ABI (include/ppfs_ecc.h) that visit only the blocks
// someone names: ppfs_ecc_scrub_list_* (a block list) and ppfs_ecc_scrub_allocated_* (the blocks whose
// bit is set in the reference's on-disk allocation bitmap, lib/bitmap/src/bitmap.cpp, read as it lies
// in the image).  The whole-image scrub stays in api.cpp.
//
// Neither reaches a row by itself: both are ppfs_ecc_decode_list_* with data == NULL, write_back = 1 and
// spill == NULL (list_path.cpp: direct for RS 2t <= 8, staged for every other codec), plus the counts.
//   list       decode the list; tally the list-order statuses (alloc_scan.hip scrub_tally_kernel)
//   allocated  1. list-decode the bitmap's own B blocks (payloads into scratch, write-back);
//              2. per piece of alloc::PIECE_BITS bits: expand the bits into the ascending block list
//                 (alloc_scan.hip; a failed bitmap block's bits count as set), read the list's length
//                 back (8 bytes, one stream synchronisation per piece);
//              3. list-decode that list;
//              4. per-bit statuses (255 for a clear bit) and counts by the tally.
// The arithmetic of the bitmap is alloc_plan.hpp, the same for the kernels and the host form.  The device
// forms' scratch is the context's (scrub_scratch below): no call allocates or frees on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "alloc_plan.hpp"
#include "ctx.hpp"
#include "kernels.hpp"
#include "list_call.hpp"

using namespace ppfs;

static_assert(sizeof(ppfs_ecc_scrub_counts) == 64, "ppfs_ecc_scrub_counts is eight 64-bit words");

namespace {

void count_host(ppfs_ecc_scrub_counts* counts, const uint8_t* st, size_t n, int slot0)
{
    uint64_t* f = &counts->ok;
    for (size_t k = 0; k < n; ++k) {
        const int slot = alloc::count_slot(st[k]);
        if (slot >= 0 && slot0 + slot < 8)
            ++f[slot0 + slot];
    }
}

// The checks of the allocated scrub that need no GPU; B = the bitmap's blocks (0 for an empty range)
int alloc_args(const ppfs_ecc_ctx* c, const void* image, size_t image_blocks, uint32_t bitmap_block, uint32_t first_block,
    size_t nbits, uint64_t& B)
{
    B = 0;
    if (!c)
        return fail(PPFS_ECC_EINVAL, "scrub allocated: null context");
    if (c->data == 0)
        return fail(PPFS_ECC_EINVAL, "scrub allocated: blocks of this codec have no payload to hold a bitmap");
    if (nbits == 0)
        return 0;
    if (!image)
        return fail(PPFS_ECC_EINVAL, "scrub allocated: null image");
    if ((uint64_t)first_block + nbits > (1ull << 32))
        return fail(PPFS_ECC_EINVAL, "scrub allocated: first_block + nbits passes 32 bits");
    B = alloc::blocks_spanned(nbits, c->data);
    if ((uint64_t)bitmap_block + B > image_blocks)
        return fail(PPFS_ECC_EINVAL, "scrub allocated: the bitmap's blocks pass the image");
    return 0;
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the host form's view of the decoded bitmap (alloc_plan.hpp Src)
struct HostSrc {
    const uint8_t* stream;
    const uint8_t* bstatus;
    uint32_t dword(uint64_t w) const
    {
        const uint8_t* p = stream + 4u * w;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    uint32_t byte(uint64_t i) const { return stream[i]; }
    uint32_t status(uint64_t b) const { return bstatus[b]; }
};

} // namespace

// The context's scrub scratch, at least `bytes` of it, for work queued on s.  It is the context's own
// memory, like the list staging: made (or replaced by a larger one; the old one stays until destroy,
// since queued work may still read it) on the context's stream, and shared by all streams, so the call
// first waits for the previous call that used it.  No call allocates or frees on the caller's stream.
int ppfs::scrub_scratch(ppfs_ecc_ctx* c, size_t bytes, hipStream_t s, uint8_t** out)
{
    if (!c->scrub_ev)
        HIP_TRY(hipEventCreateWithFlags(&c->scrub_ev, hipEventDisableTiming), "scrub event");
    if (bytes > c->scrub_bytes) {
        void* p = nullptr;
        HIP_TRY(mem_alloc(c, &p, bytes), "scrub scratch alloc");
        if (c->d_scrub)
            c->scrub_old.push_back(c->d_scrub);
        c->d_scrub = (uint8_t*)p;
        c->scrub_bytes = bytes;
    }
    if (c->scrub_ev_rec)
        HIP_TRY(hipStreamWaitEvent(s, c->scrub_ev, 0), "scrub scratch wait");
    *out = c->d_scrub;
    return 0;
}
// after the call's last use of the scratch was queued on s (also after a failure)
void ppfs::scrub_scratch_used(ppfs_ecc_ctx* c, hipStream_t s)
{
    if (hipEventRecord(c->scrub_ev, s) == hipSuccess) {
        c->scrub_ev_rec = true;
    } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s); // nothing to order the next call by: drain instead
        c->scrub_ev_rec = false;
    }
}

// ---------------------------------------------------------------------------------------
// List scrub
// ---------------------------------------------------------------------------------------
extern "C" int ppfs_ecc_scrub_list_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const uint32_t* index,
    size_t nblocks, uint8_t* status, ppfs_ecc_scrub_counts* counts)
{
    std::vector<uint8_t> own;
    if (!status && counts && nblocks) {
        own.resize(nblocks);
        status = own.data();
    }
    const int r = ppfs_ecc_decode_list_host(c, image, image_blocks, index, nblocks, nullptr, status, 1, nullptr);
    if (r || !counts)
        return r;
    *counts = ppfs_ecc_scrub_counts {};
    count_host(counts, status, nblocks, 0);
    return 0;
}

extern "C" int ppfs_ecc_scrub_list_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_status, ppfs_ecc_scrub_counts* d_counts, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_index, 1, nblocks, nullptr, false, "scrub list: null argument");
    if (r)
        return r;
    if ((uintptr_t)d_counts & 7u)
        return fail(PPFS_ECC_EINVAL, "scrub list: the counts record must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "scrub list calls cannot be captured into a graph (shared staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "scrub counts clear");
    if (nblocks == 0)
        return 0;
    uint8_t* own = nullptr; // the counts need the statuses: the context's scratch when the caller wants none
    if (!d_status && d_counts && (r = scrub_scratch(c, nblocks, s, &own)))
        return r;
    uint8_t* st = d_status ? d_status : own;
    r = ppfs_ecc_decode_list_device(c, d_image, image_blocks, d_index, nblocks, nullptr, st, 1, nullptr, stream);
    if (!r && d_counts)
        r = check_hip(ppfs_scrub_tally_launch(st, nullptr, nblocks, 0, nullptr, 0, (unsigned long long*)d_counts, 0, 4, s),
            "scrub tally");
    if (own)
        scrub_scratch_used(c, s);
    return call_queued(c, r, nblocks, stream, "scrub list (async)");
}

// ---------------------------------------------------------------------------------------
// Allocated scrub
// ---------------------------------------------------------------------------------------
extern "C" int ppfs_ecc_scrub_allocated_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, uint32_t bitmap_block,
    uint32_t first_block, size_t nbits, uint8_t* status, uint8_t* bitmap_status, ppfs_ecc_scrub_counts* counts)
{
    uint64_t B = 0;
    int r = alloc_args(c, image, image_blocks, bitmap_block, first_block, nbits, B);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_scrub_counts {};
    if (nbits == 0)
        return 0;
    const size_t ds = c->data;
    // 1. the bitmap's blocks, scrubbed like any read of them
    std::vector<uint8_t> stream(B * ds), bst(B);
    if ((r = ppfs_ecc_decode_host(c, image + (size_t)bitmap_block * c->raw, stream.data(), bst.data(), B,
             has_write_back(c) ? 1 : 0, nullptr)))
        return r;
    if (bitmap_status)
        std::memcpy(bitmap_status, bst.data(), B);
    // 2. the ascending list of the blocks to scrub
    const HostSrc src { stream.data(), bst.data() };
    std::vector<uint32_t> index;
    for (uint64_t w = 0, words = alloc::words_of(nbits); w < words; ++w)
        for (uint32_t bits = alloc::word_bits(src, w, nbits, ds, B); bits; bits &= bits - 1u)
            index.push_back(first_block + (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(bits));
    // 3. the list scrub
    std::vector<uint8_t> st(index.size());
    if ((r = ppfs_ecc_decode_list_host(c, image, image_blocks, index.data(), index.size(), nullptr, st.data(), 1, nullptr)))
        return r;
    // 4. per-bit statuses and counts
    if (status) {
        std::memset(status, PPFS_ECC_NOT_ALLOCATED, nbits);
        for (size_t k = 0; k < index.size(); ++k)
            status[index[k] - first_block] = st[k];
    }
    if (counts) {
        count_host(counts, st.data(), st.size(), 0);
        count_host(counts, bst.data(), B, alloc::SLOT_BITMAP);
        counts->not_allocated = nbits - index.size();
    }
    return 0;
}

extern "C" int ppfs_ecc_scrub_allocated_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, uint32_t bitmap_block,
    uint32_t first_block, size_t nbits, uint8_t* d_status, uint8_t* d_bitmap_status, ppfs_ecc_scrub_counts* d_counts,
    void* stream)
{
    uint64_t B = 0;
    int r = alloc_args(c, d_image, image_blocks, bitmap_block, first_block, nbits, B);
    if (r)
        return r;
    if ((uintptr_t)d_counts & 7u)
        return fail(PPFS_ECC_EINVAL, "scrub allocated: the counts record must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "scrub allocated calls cannot be captured into a graph (the host reads a count per piece)");
    unsigned long long* counts = (unsigned long long*)d_counts;
    if (counts)
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(*d_counts), s), "scrub counts clear");
    if (nbits == 0)
        return 0;

    // the call's scratch (the context's, scrub_scratch): the bitmap's block list, payload stream and
    // statuses; the scan's chunk totals and offsets and the piece's count; a piece's list and its statuses
    const size_t ds = c->data, piece_cap = std::min<uint64_t>(nbits, alloc::PIECE_BITS);
    const size_t o_bidx = 0, o_stream = round_up(o_bidx + B * 4, 256), o_bst = round_up(o_stream + B * ds, 256),
                 o_scan = round_up(o_bst + B, 256), o_total = o_scan + 2 * alloc::PIECE_CHUNKS * 4,
                 o_index = round_up(o_total + 8, 256), o_st = round_up(o_index + piece_cap * 4, 256),
                 bytes = o_st + piece_cap;
    uint8_t* scratch = nullptr;
    if ((r = scrub_scratch(c, bytes, s, &scratch)))
        return r;
    unsigned long long* bounce = nullptr; // page-locked: where the host reads a piece's count
    if (pin_alloc((void**)&bounce, 256, kPinStage) != hipSuccess)
        return fail(PPFS_ECC_ENOMEM, "scrub count bounce");
    uint32_t* d_bidx = (uint32_t*)(scratch + o_bidx);
    uint8_t *d_stream = scratch + o_stream, *d_bst = scratch + o_bst, *d_st = scratch + o_st;
    uint32_t *d_scan = (uint32_t*)(scratch + o_scan), *d_index = (uint32_t*)(scratch + o_index);
    unsigned long long* d_total = (unsigned long long*)(scratch + o_total);

    // 1. the bitmap's blocks, scrubbed like any read of them (a list, since an image row has any alignment)
    (void)((r = check_hip(ppfs_alloc_iota_launch(d_bidx, bitmap_block, B, s), "scrub bitmap list"))
        || (r = ppfs_ecc_decode_list_device(c, d_image, image_blocks, d_bidx, B, d_stream, d_bst, 1, nullptr, stream))
        || (r = check_hip(ppfs_scrub_tally_launch(d_bst, d_bidx, B, bitmap_block, d_bitmap_status, B, counts, alloc::SLOT_BITMAP,
                              3, s),
                "scrub bitmap tally")));
    for (uint64_t p = 0, np = alloc::pieces_of(nbits); p < np && !r; ++p) {
        const alloc::Piece piece = alloc::piece_of(nbits, p);
        // 2. the piece's bits -> its ascending block list; the host needs its length to size the list call
        if ((r = check_hip(ppfs_alloc_expand_launch(d_stream, d_bst, B, ds, nbits, first_block, p, d_scan, d_total, d_index,
                               counts, s),
                 "scrub bitmap expand")))
            break;
        if (d_status && (r = check_hip(hipMemsetAsync(d_status + piece.bit0, PPFS_ECC_NOT_ALLOCATED, piece.bits, s), "scrub status fill")))
            break;
        if ((r = check_hip(dma_async(bounce, d_total, 8, hipMemcpyDeviceToHost, s), "scrub count D2H"))
            || (r = check_hip(hipStreamSynchronize(s), "scrub sync")))
            break;
        const size_t n = (size_t)*bounce;
        if (n == 0)
            continue;
        if (n > piece.bits) {
            r = fail(PPFS_ECC_EHIP, "scrub allocated: a piece's count passes its bits");
            break;
        }
        // 3. the list scrub, 4. per-bit statuses and counts
        (void)((r = ppfs_ecc_decode_list_device(c, d_image, image_blocks, d_index, n, nullptr, d_st, 1, nullptr, stream))
            || (r = check_hip(ppfs_scrub_tally_launch(d_st, d_index, n, first_block + (uint32_t)piece.bit0,
                                  d_status ? d_status + piece.bit0 : nullptr, piece.bits, counts, 0, 4, s),
                    "scrub tally")));
    }
    scrub_scratch_used(c, s);
    if (r)
        (void)hipStreamSynchronize(s); // a failure may have left the bounce's copy queued
    pin_free(bounce, 256, kPinStage); // its last copy completed at the last piece's synchronisation
    return call_queued(c, r, nbits, stream, "scrub allocated (async)");
}
