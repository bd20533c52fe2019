// list_path.cpp -- the block-list entry points of the ppfs_ecc C ABI (include/ppfs_ecc.h):
// decode / encode / write of "these N block indices of this image, in this order", the call
// FileIO's BlockIndexIterator loop (lib/file_io/src/file_io.cpp:27-35, 53-69) needs for a file
// whose blocks lie wherever the bitmap allocator put them.
//
// Device forms: a frame (ListCall) around one straight sequence of operations per piece of listed rows
// (PieceIO; both in list_call.hpp, both used by the byte-extent calls of extent_path.cpp too):
//   decode: fetch, decode, marks    encode: fetch if the encode keeps old bits, encode    write: fetch, write, marks
// PieceIO is the one place where the two ways to reach the rows part:
//   operation     staged (every codec)                                direct (RS(255, 255-2t), 2t <= 8)
//   fetch         gather into the row staging (vote.hip)              nothing
//   decode        contiguous decode of the staging; scatter of the    one list decode (rs_wg_list.hpp), and the
//                 corrected rows (status 1) when writing back         spill memset
//   old payloads  contiguous decode into P without status (not when   list decode into P and the status array,
//                 the data size is 0)                                 nothing written back
//   encode        contiguous encode into the staging; scatter of      one list encode: codeword i stored at
//                 every row                                           image + index[i] * 255
//   write         contiguous write of the staging; scatter of the     status-only list decode (not when the statuses
//                 rows with a status other than 5                     are known or unwanted), list encode
//   marks         list_oob_kernel: status 9, zero payload             nothing: the kernels made them
// Staged lists longer than one piece (list_plan.hpp piece_blocks) go piece by piece through the context's
// shared staging, which list_ev orders between calls.  A list call is direct when the context is
// (PPFS_ECC_LIST_DIRECT=0 at ppfs_ecc_create keeps it staged) and the caller's arrays meet the kernels'
// 16-byte rule; it is one piece without staging or list_ev, framed like a contiguous device call.
// Host forms: the list is cut into runs without a repeated index, each run is gathered on the CPU
// and handed to the contiguous host call, and the rows that changed are copied back.
// The arithmetic of both is in list_plan.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
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

// The gate of a direct list call: the 16-byte rule of the contiguous RS decode and encode
// (ppfs_ecc_decode_device, ppfs_ecc_encode_device); a call that breaks it takes the staged path, which
// refuses it as before
bool list_direct_args(const ppfs_ecc_ctx* c, const void* d_data, const void* d_status)
{
    return c->list_direct && (((uintptr_t)d_data | (uintptr_t)d_status) & 15u) == 0;
}

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

size_t ppfs::piece_of(ppfs_ecc_ctx* c) { return piece_blocks(ppfs_ecc_host_chunk_blocks(c), c->raw); }

int ppfs::entry_args(const ppfs_ecc_ctx* c, const void* image, size_t image_blocks, const void* entries, unsigned align,
    size_t n, const void* buf, bool buf_needed, const char* what)
{
    if (!c || (n && (!entries || ((uintptr_t)entries & (align - 1)) || (image_blocks && !image) || (buf_needed && !buf))))
        return fail(PPFS_ECC_EINVAL, what);
    return 0;
}

// The frame of one device call (list_call.hpp).  The staging is shared by every stream of the context,
// so a call that uses it first waits for the event recorded after the previous such call's last kernel
// and records it again after its own.
int ppfs::ListCall::begin()
{
    if (stream_capturing(s()))
        return fail(PPFS_ECC_ENOTSUP, (std::string(kind) + " calls cannot be captured into a graph (shared staging)").c_str());
    if (staging) {
        int r = ensure_stage(c);
        if (r)
            return r;
    }
    (void)call_ordered(c, nblocks, stream);
    if (staging && c->list_ev_rec)
        HIP_TRY(hipStreamWaitEvent(s(), c->list_ev, 0), "list staging wait");
    return 0;
}

int ppfs::ListCall::end(int r, const char* what)
{
    if (!staging)
        return call_queued(c, r, nblocks, stream, what);
    // also after a failure: pieces queued before it may still use the staging
    if (hipEventRecord(c->list_ev, s()) == hipSuccess) {
        c->list_ev_rec = true;
    } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s()); // nothing to order the next call by: drain instead
        c->list_ev_rec = false;
    }
    return call_queued(c, r, nblocks, stream, what);
}

// ---------------------------------------------------------------------------------------
// One piece of listed rows (list_call.hpp): the table above
// ---------------------------------------------------------------------------------------
int ppfs::PieceIO::fetch(const uint32_t* ix, size_t nb)
{
    if (direct)
        return 0;
    return check_hip(ppfs_gather_blocks_launch(image, blocks, ix, (uint32_t)nb, c->raw, rows(), s()), "list gather");
}

int ppfs::PieceIO::decode(const uint32_t* ix, size_t nb, uint8_t* data, uint8_t* st, bool wb, uint8_t* spill)
{
    if (direct) {
        if (spill) // n = 255: one count byte per entry, always zero (a write-back never passes the block's end)
            HIP_TRY(hipMemsetAsync(spill, 0, nb * spill_bytes(c), s()), "list spill");
        return check_hip(ppfs_rs_list_decode(c->rs_t2, image, blocks, ix, data, st, nb, c->d_tables, wb ? 1 : 0, s()),
            "rs list decode");
    }
    if (!st && wb) // the scatter selects by status: the context's own array when the caller wants none
        st = own_status();
    int r = ppfs_ecc_decode_device(c, rows(), data, st, nb, wb ? 1 : 0, spill, stream);
    if (!r && wb)
        r = check_hip(ppfs_scatter_blocks_launch(rows(), image, blocks, ix, st, 1, (uint32_t)nb, c->raw, s()), "list scatter");
    return r;
}

int ppfs::PieceIO::old_payloads(const uint32_t* ix, size_t nb, uint8_t* P, uint8_t* st)
{
    if (direct) { // the statuses come with the payloads (9 and zeros for an entry out of range)
        old_status_known = true;
        return decode(ix, nb, P, st, false, nullptr);
    }
    // where the old block fails its check (status 5 in write()) the row is not scattered and what P
    // holds for it does not matter
    return c->data ? ppfs_ecc_decode_device(c, rows(), P, nullptr, nb, 0, nullptr, stream) : 0;
}

int ppfs::PieceIO::encode(const uint32_t* ix, size_t nb, const uint8_t* data)
{
    if (direct)
        return check_hip(ppfs_rs_list_encode(c->rs_t2, data, image, blocks, ix, nb, c->d_tables, s()), "rs list encode");
    int r = ppfs_ecc_encode_device(c, data, rows(), nb, stream);
    if (!r)
        r = check_hip(ppfs_scatter_blocks_launch(rows(), image, blocks, ix, nullptr, 0, (uint32_t)nb, c->raw, s()), "list scatter");
    return r;
}

int ppfs::PieceIO::write(const uint32_t* ix, size_t nb, const uint8_t* data, uint8_t* st)
{
    if (direct) {
        // the old blocks' statuses (0 / 1, 9 for an entry out of range) by the list decode, which changes
        // nothing; then the new codewords, whatever the status was: RS needs nothing else of the old block
        // (rs_block_device.cpp:61-93)
        int r = st && !old_status_known ? decode(ix, nb, nullptr, st, false, nullptr) : 0;
        old_status_known = false;
        return r ? r : encode(ix, nb, data);
    }
    if (!st) // the scatter selects by status
        st = own_status();
    int r = ppfs_ecc_write_device(c, data, rows(), st, nb, stream);
    if (!r)
        r = check_hip(ppfs_scatter_blocks_launch(rows(), image, blocks, ix, st, 2, (uint32_t)nb, c->raw, s()), "list scatter");
    return r;
}

int ppfs::PieceIO::marks(const uint32_t* ix, size_t nb, uint8_t* st, uint8_t* data)
{
    if (direct)
        return 0;
    return check_hip(ppfs_list_oob_launch(ix, (uint32_t)nb, blocks, st, data, data ? c->data : 0, s()), "list range marks");
}

// ---------------------------------------------------------------------------------------
// Device forms
// ---------------------------------------------------------------------------------------
extern "C" int ppfs_ecc_decode_list_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const uint32_t* d_index,
    size_t nblocks, uint8_t* d_data, uint8_t* d_status, int write_back, uint8_t* d_spill, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_index, 1, nblocks, d_data, false, "decode list: null argument");
    if (r || nblocks == 0)
        return r;
    const bool direct = list_direct_args(c, d_data, d_status), wb = write_back && has_write_back(c);
    ListCall call { c, stream, nblocks, "list", !direct };
    if ((r = call.begin()))
        return r;
    PieceIO io { c, d_image, image_blocks, stream, direct };
    for (size_t off = 0, piece = call.piece(); off < nblocks && !r; off += piece) {
        const size_t nb = std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        uint8_t* st = d_status ? d_status + off : nullptr;
        uint8_t* dd = d_data ? d_data + off * c->data : nullptr;
        uint8_t* sp = d_spill ? d_spill + off * spill_bytes(c) : nullptr;
        (void)((r = io.fetch(ix, nb)) || (r = io.decode(ix, nb, dd, st, wb, sp)) || (r = io.marks(ix, nb, st, dd)));
    }
    return call.end(r, "decode list (async)");
}

extern "C" int ppfs_ecc_encode_list_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, size_t nblocks, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_index, 1, nblocks, d_data, c && c->data, "encode list: null argument");
    if (r || nblocks == 0)
        return r;
    const bool direct = list_direct_args(c, d_data, nullptr);
    ListCall call { c, stream, nblocks, "list", !direct };
    if ((r = call.begin()))
        return r;
    PieceIO io { c, d_image, image_blocks, stream, direct };
    for (size_t off = 0, piece = call.piece(); off < nblocks && !r; off += piece) {
        const size_t nb = std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        const uint8_t* dd = d_data ? d_data + off * c->data : nullptr;
        if (!(r = encode_keeps_old_bits(c) ? io.fetch(ix, nb) : 0))
            r = io.encode(ix, nb, dd);
    }
    return call.end(r, "encode list (async)");
}

extern "C" int ppfs_ecc_write_list_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_image, size_t image_blocks,
    const uint32_t* d_index, uint8_t* d_status, size_t nblocks, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_index, 1, nblocks, d_data, c && c->data, "write list: null argument");
    if (r || nblocks == 0)
        return r;
    const bool direct = list_direct_args(c, d_data, d_status);
    ListCall call { c, stream, nblocks, "list", !direct };
    if ((r = call.begin()))
        return r;
    PieceIO io { c, d_image, image_blocks, stream, direct };
    for (size_t off = 0, piece = call.piece(); off < nblocks && !r; off += piece) {
        const size_t nb = std::min(piece, nblocks - off);
        const uint32_t* ix = d_index + off;
        uint8_t* st = d_status ? d_status + off : nullptr;
        const uint8_t* dd = d_data ? d_data + off * c->data : nullptr;
        (void)((r = io.fetch(ix, nb)) || (r = io.write(ix, nb, dd, st)) || (r = io.marks(ix, nb, st, nullptr)));
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
    const size_t raw = c->raw, ds = c->data, sb = spill_bytes(c);
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
