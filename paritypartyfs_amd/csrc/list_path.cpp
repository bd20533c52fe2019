// list_path.cpp -- the block-list entry points of the ppfs_ecc C ABI (include/ppfs_ecc.h):
// decode / encode / write of "these N block indices of this image, in this order", the call
// FileIO's BlockIndexIterator loop (lib/file_io/src/file_io.cpp:27-35, 53-69) needs for a file
// whose blocks lie wherever the bitmap allocator put them.
//
// Device forms: the listed rows are gathered into a dense, context-owned staging copy
// (vote.hip gather_blocks_kernel), the unchanged codec kernels run on that copy through the
// contiguous entry points, and the rows that changed are scattered back (scatter_blocks_kernel).
// Lists longer than one piece (list_plan.hpp piece_blocks) go piece by piece on the caller's stream.
// RS(255, 255-2t), 2t <= 8 decodes a list in one kernel instead (rs_wg_list.hpp: the rows are fetched
// from the image by the codec kernel's loader and corrected in place): no staging, no pieces, no
// list_ev, framed like a contiguous device call.  PPFS_ECC_LIST_DIRECT=0 at ppfs_ecc_create keeps such
// a context on the staged path.  Such a context also encodes and writes a list directly: the list encode
// (rs_wg_list.hpp rs_wg_encode_list_kernel) stores codeword i at image + index[i] * 255 itself, and an RS
// write needs nothing of the old block but its status (rs_block_device.cpp:61-93), which the list
// decode gives without touching the image -- two kernels on the caller's stream in place of gather,
// decode, encode, scatter and range marks.
// Host forms: the list is cut into runs without a repeated index, each run is gathered on the CPU
// and handed to the contiguous host call, and the rows that changed are copied back.
// The arithmetic of both is in list_plan.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "kernels.hpp"
#include "list_call.hpp"
#include "list_plan.hpp"

using namespace ppfs;
using namespace ppfs::listplan;

namespace {

// Does an encode leave bits of the raw block as they were (ppfs_ecc_encode_device)?  Then the old
// rows are gathered before the codec runs: Hamming's bits after the last data bit, the tail bits of
// a CRC whose degree is no multiple of 8, and the parity byte, of which the encode only ever flips
// bit 0 (parity_block_device.cpp:49-54).
bool encode_keeps_old_bits(const ppfs_ecc_ctx* c)
{
    return c->p.ecc_type == PPFS_ECC_HAMMING || c->p.ecc_type == PPFS_ECC_PARITY
        || (c->p.ecc_type == PPFS_ECC_CRC && c->crc_n % 8 != 0);
}

} // namespace

bool ppfs::has_write_back(const ppfs_ecc_ctx* c)
{
    return c->p.ecc_type == PPFS_ECC_REED_SOLOMON || c->p.ecc_type == PPFS_ECC_HAMMING;
}

size_t ppfs::piece_of(ppfs_ecc_ctx* c) { return piece_blocks(ppfs_ecc_host_chunk_blocks(c), c->raw); }

namespace {

// The staging of the list calls, made once per context (the piece size does not change)
int ensure_stage(ppfs_ecc_ctx* c)
{
    if (c->d_list)
        return 0;
    const StageLayout L = stage_layout(piece_of(c), c->raw);
    if (!c->list_ev)
        HIP_TRY(hipEventCreateWithFlags(&c->list_ev, hipEventDisableTiming), "list event");
    HIP_TRY(mem_alloc(c, (void**)&c->d_list, L.total), "list staging alloc");
    c->list_bytes = L.total;
    c->list_status_off = L.status;
    return 0;
}

} // namespace

// One device list call: the common frame around its pieces (list_call.hpp).  The staging is shared by
// every stream of the context, so the call first waits for the event recorded after the previous list
// call's last kernel and records it again after its own.
int ppfs::ListCall::begin()
{
    int r = ensure_stage(c);
    if (r)
        return r;
    (void)call_ordered(c, nblocks, stream);
    if (c->list_ev_rec)
        HIP_TRY(hipStreamWaitEvent(s, c->list_ev, 0), "list staging wait");
    return 0;
}

int ppfs::ListCall::end(int r, const char* what)
{
    // also after a failure: pieces queued before it may still use the staging
    if (hipEventRecord(c->list_ev, s) == hipSuccess) {
        c->list_ev_rec = true;
    } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s); // nothing to order the next call by: drain instead
        c->list_ev_rec = false;
    }
    return call_queued(c, r, nblocks, stream, what);
}

// ---------------------------------------------------------------------------------------
// The direct list decode (ctx.hpp)
// ---------------------------------------------------------------------------------------
bool ppfs::list_direct_args(const ppfs_ecc_ctx* c, const void* d_data, const void* d_status)
{
    // the rule of the contiguous RS decode (ppfs_ecc_decode_device); a call that breaks it takes the
    // staged path, which refuses it as before
    return c->list_direct && (((uintptr_t)d_data | (uintptr_t)d_status) & 15u) == 0;
}

int ppfs::decode_list_direct(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_data, uint8_t* d_status, int write_back, uint8_t* d_spill, hipStream_t s)
{
    if (d_spill) // n = 255: one count byte per entry, always zero (a write-back never passes the block's end)
        HIP_TRY(hipMemsetAsync(d_spill, 0, nblocks, s), "list spill");
    return check_hip(ppfs_rs_list_decode(c->rs_t2, d_image, image_blocks, d_index, d_data, d_status, nblocks, c->d_tables,
                         write_back ? 1 : 0, s),
        "rs list decode");
}

// The direct list encode.  Its gate is list_direct_args too: d_data by the rule of the contiguous RS
// encode (ppfs_ecc_encode_device), a write's d_status by the decode's.
int ppfs::encode_list_direct(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, size_t nblocks, hipStream_t s)
{
    return check_hip(ppfs_rs_list_encode(c->rs_t2, d_data, d_image, image_blocks, d_index, nblocks, c->d_tables, s),
        "rs list encode");
}

namespace {

int list_args(ppfs_ecc_ctx* c, const void* d_image, size_t image_blocks, const void* d_index, size_t nblocks,
    const void* d_data, bool data_required, void* stream, const char* what)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, what);
    if (nblocks && (!d_index || (image_blocks && !d_image) || (data_required && c->data && !d_data)))
        return fail(PPFS_ECC_EINVAL, what);
    if (nblocks && stream_capturing((hipStream_t)stream))
        return fail(PPFS_ECC_ENOTSUP, "list calls cannot be captured into a graph (shared staging)");
    return 0;
}

} // namespace

extern "C" int ppfs_ecc_decode_list_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_data, uint8_t* d_status, int write_back, uint8_t* d_spill, void* stream)
{
    int r = list_args(c, d_image, image_blocks, d_index, nblocks, d_data, false, stream, "decode list: null argument");
    if (r || nblocks == 0)
        return r;
    if (list_direct_args(c, d_data, d_status)) {
        (void)call_ordered(c, nblocks, stream);
        r = decode_list_direct(c, d_image, image_blocks, d_index, nblocks, d_data, d_status, write_back, d_spill,
            (hipStream_t)stream);
        return call_queued(c, r, nblocks, stream, "decode list (async)");
    }
    ListCall call { c, (hipStream_t)stream, stream, nblocks };
    if ((r = call.begin()))
        return r;
    const size_t piece = piece_of(c), sb = 256 - std::min<size_t>(c->raw, 255);
    const bool wb = write_back && has_write_back(c);
    uint8_t* rows = c->d_list;
    for (size_t off = 0; off < nblocks && !r; off += piece) {
        const uint32_t nb = (uint32_t)std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        // the scatter selects by status: the context's own array when the caller wants none
        uint8_t* st = d_status ? d_status + off : (wb ? c->d_list + c->list_status_off : nullptr);
        uint8_t* dd = d_data ? d_data + off * c->data : nullptr;
        r = check_hip(ppfs_gather_blocks_launch(d_image, image_blocks, ix, nb, c->raw, rows, call.s), "list gather");
        if (!r)
            r = ppfs_ecc_decode_device(c, rows, dd, st, nb, wb ? 1 : 0, d_spill ? d_spill + off * sb : nullptr, stream);
        if (!r && wb)
            r = check_hip(ppfs_scatter_blocks_launch(rows, d_image, image_blocks, ix, st, 1, nb, c->raw, call.s),
                "list scatter");
        if (!r)
            r = check_hip(
                ppfs_list_oob_launch(ix, nb, image_blocks, d_status ? st : nullptr, dd, c->data, call.s), "list range marks");
    }
    return call.end(r, "decode list (async)");
}

extern "C" int ppfs_ecc_encode_list_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, size_t nblocks, void* stream)
{
    int r = list_args(c, d_image, image_blocks, d_index, nblocks, d_data, true, stream, "encode list: null argument");
    if (r || nblocks == 0)
        return r;
    if (list_direct_args(c, d_data, nullptr)) {
        (void)call_ordered(c, nblocks, stream);
        r = encode_list_direct(c, d_data, d_image, image_blocks, d_index, nblocks, (hipStream_t)stream);
        return call_queued(c, r, nblocks, stream, "encode list (async)");
    }
    ListCall call { c, (hipStream_t)stream, stream, nblocks };
    if ((r = call.begin()))
        return r;
    const size_t piece = piece_of(c);
    uint8_t* rows = c->d_list;
    for (size_t off = 0; off < nblocks && !r; off += piece) {
        const uint32_t nb = (uint32_t)std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        if (encode_keeps_old_bits(c))
            r = check_hip(ppfs_gather_blocks_launch(d_image, image_blocks, ix, nb, c->raw, rows, call.s), "list gather");
        if (!r)
            r = ppfs_ecc_encode_device(c, d_data ? d_data + off * c->data : nullptr, rows, nb, stream);
        if (!r)
            r = check_hip(ppfs_scatter_blocks_launch(rows, d_image, image_blocks, ix, nullptr, 0, nb, c->raw, call.s),
                "list scatter");
    }
    return call.end(r, "encode list (async)");
}

extern "C" int ppfs_ecc_write_list_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, uint8_t* d_status, size_t nblocks, void* stream)
{
    int r = list_args(c, d_image, image_blocks, d_index, nblocks, d_data, true, stream, "write list: null argument");
    if (r || nblocks == 0)
        return r;
    if (list_direct_args(c, d_data, d_status)) {
        // the old blocks' statuses (0 / 1, 9 for an entry out of range) by the list decode, which
        // changes nothing; then the new codewords, whatever the status was.  Without d_status the
        // encode alone: RS needs nothing else of the old block.
        hipStream_t s = (hipStream_t)stream;
        (void)call_ordered(c, nblocks, stream);
        if (d_status)
            r = decode_list_direct(c, d_image, image_blocks, d_index, nblocks, nullptr, d_status, 0, nullptr, s);
        if (!r)
            r = encode_list_direct(c, d_data, d_image, image_blocks, d_index, nblocks, s);
        return call_queued(c, r, nblocks, stream, "write list (async)");
    }
    ListCall call { c, (hipStream_t)stream, stream, nblocks };
    if ((r = call.begin()))
        return r;
    const size_t piece = piece_of(c);
    uint8_t* rows = c->d_list;
    for (size_t off = 0; off < nblocks && !r; off += piece) {
        const uint32_t nb = (uint32_t)std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        uint8_t* st = d_status ? d_status + off : c->d_list + c->list_status_off;
        r = check_hip(ppfs_gather_blocks_launch(d_image, image_blocks, ix, nb, c->raw, rows, call.s), "list gather");
        if (!r)
            r = ppfs_ecc_write_device(c, d_data ? d_data + off * c->data : nullptr, rows, st, nb, stream);
        if (!r)
            r = check_hip(ppfs_scatter_blocks_launch(rows, d_image, image_blocks, ix, st, 2, nb, c->raw, call.s),
                "list scatter");
        if (!r && d_status)
            r = check_hip(ppfs_list_oob_launch(ix, nb, image_blocks, st, nullptr, 0, call.s), "list range marks");
    }
    return call.end(r, "write list (async)");
}

// ---------------------------------------------------------------------------------------
// Host forms.  The chunk pipeline (host_path.cpp) is used as it is, on a gathered copy of each run.
// ---------------------------------------------------------------------------------------
namespace {

struct HostList {
    Op op;
    const uint8_t* data_in; // encode, write
    uint8_t* data_out;      // decode
    uint8_t* image;
    size_t image_blocks;
    const uint32_t* index;
    size_t nblocks;
    uint8_t* status;
    int write_back;
    uint8_t* spill;
};

int host_list_run(ppfs_ecc_ctx* c, const HostList& h)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, "list (host): null context");
    if (h.nblocks == 0)
        return 0;
    if (!h.index || (h.image_blocks && !h.image) || (h.op != OP_DECODE && c->data && !h.data_in))
        return fail(PPFS_ECC_EINVAL, "list (host): null argument");
    const size_t raw = c->raw, ds = c->data, sb = 256 - std::min<size_t>(raw, 255);
    const size_t max_run = 8 * ppfs_ecc_host_chunk_blocks(c); // bounds the gathered copy; any cut gives the same result
    const bool wb = h.op == OP_DECODE && h.write_back && has_write_back(c);
    const bool need_rows = h.op != OP_ENCODE || encode_keeps_old_bits(c);
    std::vector<uint8_t> rows, st_own;
    for (size_t start = 0; start < h.nblocks;) {
        const size_t end = run_end(h.index, h.nblocks, start, h.image_blocks, max_run);
        const size_t m = end - start;
        const uint32_t* ix = h.index + start;
        if (rows.size() < m * raw)
            rows.resize(m * raw);
        if (need_rows)
            gather_rows_cpu(h.image, h.image_blocks, ix, m, raw, rows.data());
        uint8_t* st = h.status ? h.status + start : nullptr;
        if (!st && (wb || h.op == OP_WRITE)) {
            st_own.resize(std::max(st_own.size(), m));
            st = st_own.data();
        }
        int r = 0;
        switch (h.op) {
        case OP_DECODE:
            r = ppfs_ecc_decode_host(c, rows.data(), h.data_out ? h.data_out + start * ds : nullptr, st, m, wb ? 1 : 0,
                h.spill ? h.spill + start * sb : nullptr);
            break;
        case OP_ENCODE:
            r = ppfs_ecc_encode_host(c, h.data_in ? h.data_in + start * ds : nullptr, rows.data(), m);
            break;
        case OP_WRITE:
            r = ppfs_ecc_write_host(c, h.data_in ? h.data_in + start * ds : nullptr, rows.data(), st, m);
            break;
        }
        if (r)
            return r;
        for (uint32_t i : copy_back_list(h.op, wb, ix, m, h.image_blocks, st))
            std::memcpy(h.image + (size_t)ix[i] * raw, rows.data() + (size_t)i * raw, raw);
        mark_out_of_range(ix, m, h.image_blocks, h.status ? st : nullptr,
            h.op == OP_DECODE && h.data_out ? h.data_out + start * ds : nullptr, ds);
        start = end;
    }
    return 0;
}

} // namespace

extern "C" int ppfs_ecc_decode_list_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const uint32_t* index,
    size_t nblocks, uint8_t* data, uint8_t* status, int write_back, uint8_t* spill)
{
    return host_list_run(c, HostList { OP_DECODE, nullptr, data, image, image_blocks, index, nblocks, status, write_back, spill });
}

extern "C" int ppfs_ecc_encode_list_host(ppfs_ecc_ctx* c, const uint8_t* data, uint8_t* image, size_t image_blocks,
    const uint32_t* index, size_t nblocks)
{
    return host_list_run(c, HostList { OP_ENCODE, data, nullptr, image, image_blocks, index, nblocks, nullptr, 0, nullptr });
}

extern "C" int ppfs_ecc_write_list_host(ppfs_ecc_ctx* c, const uint8_t* data, uint8_t* image, size_t image_blocks,
    const uint32_t* index, uint8_t* status, size_t nblocks)
{
    return host_list_run(c, HostList { OP_WRITE, data, nullptr, image, image_blocks, index, nblocks, status, 0, nullptr });
}
