// extent_path.cpp -- the byte-extent entry points of the ppfs_ecc C ABI (include/ppfs_ecc.h): reads and
// writes of "these n byte ranges of those blocks", a batch of readBlock({block, offset}, length) /
// writeBlock(bytes, {block, offset}) calls (rs_block_device.cpp:25-93, crc_block_device.cpp:69-122,
// hamming_block_device.cpp:111-162, parity_block_device.cpp:31-88) -- what FileIO::readFile / writeFile
// (lib/file_io/src/file_io.cpp:24-42, 50-88) issue for a file range that starts and ends mid-block, and
// what the inode table, bitmap and directory code issue for their few bytes.
//
// Device forms: the block-list calls' frame and piece of listed rows (ListCall, PieceIO: list_call.hpp,
// the table in list_path.cpp), in pieces of the same size, plus a second staging for the decoded
// payloads P of a piece and the staged index of its entries.  An entry that is invalid is staged as
// index 0xFFFFFFFF, which every way to reach the rows treats as out of range: status 9, a zero payload,
// nothing stored.
//   read   index, fetch, decode (rows -> P, status, write_back), pack P into the caller's buffer,
//          status out, marks
//   write  index, fetch, old payloads (rows -> P), overlay the caller's bytes onto P,
//          write (P -> rows, status), status out, marks
// The piece is direct when the context is (ctx.hpp list_direct): P and the status array the codec gets are
// 16-byte aligned by construction.  Every extent call uses the shared staging, the context's own status
// array (in the row staging) included, so every one is ordered by list_ev.
// Host forms: the list is cut into runs without a repeated valid block, each run is gathered on the
// CPU, goes through the contiguous host calls and is copied back.  The arithmetic of both is in
// extent_plan.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "extent_plan.hpp"
#include "kernels.hpp"
#include "list_call.hpp"
#include "list_plan.hpp"

using namespace ppfs;
using namespace ppfs::listplan;
using namespace ppfs::extplan;

namespace {

// The extent calls' own staging, made at their first use (after ListCall::begin made the rows')
int ensure_ext_stage(ppfs_ecc_ctx* c)
{
    if (c->d_ext)
        return 0;
    const ExtStageLayout L = ext_stage_layout(piece_of(c), c->data);
    HIP_TRY(mem_alloc(c, (void**)&c->d_ext, L.total), "extent staging alloc");
    c->ext_bytes = L.total;
    c->ext_index_off = L.index;
    return 0;
}

// What a piece of a device extent call works with besides its rows
struct ExtStage {
    ppfs_ecc_ctx* c;
    hipStream_t s;
    uint8_t* P;
    uint32_t* idx;
    ExtStage(ppfs_ecc_ctx* ctx, hipStream_t stream)
        : c(ctx), s(stream), P(ctx->d_ext), idx((uint32_t*)(ctx->d_ext + ctx->ext_index_off))
    {
    }
    int index(const ppfs_ecc_extent* ex, uint32_t nb, size_t blocks, size_t buf_bytes) const
    {
        return check_hip(ppfs_extent_index_launch(ex, nb, blocks, c->data, buf_bytes, idx, s), "extent index");
    }
    // to_stage 0: pack P's bytes into buf, selected by st; 1: overlay buf's bytes, which the kernel only reads, onto P
    int copy(int to_stage, const ppfs_ecc_extent* ex, const uint8_t* st, uint32_t nb, const uint8_t* buf, size_t buf_bytes) const
    {
        return check_hip(ppfs_extent_copy_launch(to_stage, ex, idx, st, nb, c->data, P, c->ext_index_off,
                             const_cast<uint8_t*>(buf), buf_bytes, s),
            to_stage ? "extent overlay" : "extent pack");
    }
    // the codecs want a 16-byte aligned status array (RS, Hamming), and the pack and the scatter select
    // by status: the caller's where it is aligned, else the context's own, copied out afterwards
    uint8_t* status_for(uint8_t* d_status, size_t off) const
    {
        return d_status && (((uintptr_t)d_status & 15u) == 0) ? d_status + off : c->d_list + c->list_status_off;
    }
    int status_out(const uint8_t* st, uint8_t* out, uint32_t nb) const // out: the caller's piece, or null
    {
        return out && st != out ? check_hip(dma_async(out, st, nb, hipMemcpyDeviceToDevice, s), "extent status copy") : 0;
    }
};

} // namespace

extern "C" int ppfs_ecc_read_extents_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks,
    const ppfs_ecc_extent* d_ext, size_t n, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, int write_back, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_ext, 8, n, d_out, out_bytes != 0, "read extents: null or misaligned argument");
    if (r || n == 0)
        return r;
    ListCall call { c, stream, n, "extent", true };
    if ((r = call.begin()))
        return r;
    if (!(r = ensure_ext_stage(c))) {
        const ExtStage x(c, call.s());
        PieceIO io { c, d_image, image_blocks_seen(image_blocks), stream, c->list_direct };
        const bool wb = write_back && has_write_back(c);
        for (size_t off = 0, piece = call.piece(); off < n && !r; off += piece) {
            const uint32_t nb = (uint32_t)std::min(piece, n - off);
            const ppfs_ecc_extent* ex = d_ext + off;
            uint8_t* st = x.status_for(d_status, off);
            uint8_t* out_st = d_status ? d_status + off : nullptr;
            (void)((r = x.index(ex, nb, io.blocks, out_bytes)) || (r = io.fetch(x.idx, nb))
                || (r = io.decode(x.idx, nb, c->data ? x.P : nullptr, st, wb, nullptr))
                || (r = x.copy(0, ex, st, nb, d_out, out_bytes)) || (r = x.status_out(st, out_st, nb))
                || (r = io.marks(x.idx, nb, out_st, nullptr)));
        }
    }
    return call.end(r, "read extents (async)");
}

// The write piece loop, its overlay step a parameter (list_call.hpp): between "old payloads" and "write" the caller
// puts its bytes onto P.  buf_bytes: the packed buffer the entries' pos and length are checked against.
int ppfs::write_extents_pieces(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_extent* d_ext, size_t n,
    size_t buf_bytes, uint8_t* d_status, void* stream, const ExtOverlay& overlay, const char* what)
{
    ListCall call { c, stream, n, "extent", true };
    int r = call.begin();
    if (r)
        return r;
    if (!(r = ensure_ext_stage(c))) {
        const ExtStage x(c, call.s());
        PieceIO io { c, d_image, image_blocks_seen(image_blocks), stream, c->list_direct };
        for (size_t off = 0, piece = call.piece(); off < n && !r; off += piece) {
            const uint32_t nb = (uint32_t)std::min(piece, n - off);
            const ppfs_ecc_extent* ex = d_ext + off;
            uint8_t* st = x.status_for(d_status, off);
            uint8_t* out_st = d_status ? d_status + off : nullptr;
            (void)((r = x.index(ex, nb, io.blocks, buf_bytes)) || (r = io.fetch(x.idx, nb))
                || (r = io.old_payloads(x.idx, nb, x.P, st))
                || (r = overlay(ExtPiece { ex, x.idx, nb, x.P, c->ext_index_off, off, call.s() }))
                || (r = io.write(x.idx, nb, c->data ? x.P : nullptr, st)) || (r = x.status_out(st, out_st, nb))
                || (r = io.marks(x.idx, nb, out_st, nullptr)));
        }
    }
    return call.end(r, what);
}

extern "C" int ppfs_ecc_write_extents_device(ppfs_ecc_ctx* c, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_extent* d_ext, size_t n, uint8_t* d_status, void* stream)
{
    int r = entry_args(c, d_image, image_blocks, d_ext, 8, n, d_in, in_bytes != 0, "write extents: null or misaligned argument");
    if (r || n == 0)
        return r;
    // the caller's bytes: extent_copy<true>, nothing where there are none
    const ExtOverlay overlay = [&](const ExtPiece& p) {
        return check_hip(ppfs_extent_copy_launch(1, p.ex, p.idx, nullptr, p.nb, c->data, p.P, p.P_cap, const_cast<uint8_t*>(d_in),
                             in_bytes, p.s),
            "extent overlay");
    };
    return write_extents_pieces(c, d_image, image_blocks, d_ext, n, in_bytes, d_status, stream, overlay, "write extents (async)");
}

// ---------------------------------------------------------------------------------------
// Host forms.  The chunk pipeline (host_path.cpp) is used as it is, on a gathered copy of each run.
// ---------------------------------------------------------------------------------------
namespace {

struct HostExtents {
    bool write;
    const uint8_t* in; // write
    uint8_t* out;      // read
    size_t buf_bytes;
    uint8_t* image;
    size_t image_blocks;
    const ppfs_ecc_extent* ext;
    size_t n;
    uint8_t* status;
    int write_back;
};

int host_extents_run(ppfs_ecc_ctx* c, const HostExtents& h)
{
    int r = entry_args(c, h.image, h.image_blocks, h.ext, 8, h.n, h.write ? h.in : h.out, h.buf_bytes != 0,
        "extents (host): null or misaligned argument");
    if (r || h.n == 0)
        return r;
    const size_t raw = c->raw, ds = c->data, blocks = image_blocks_seen(h.image_blocks);
    const size_t max_run = 8 * ppfs_ecc_host_chunk_blocks(c); // bounds the gathered copy; any cut gives the same result
    const bool wb = !h.write && h.write_back && has_write_back(c);
    std::vector<uint32_t> ix(h.n);
    for (size_t i = 0; i < h.n; ++i)
        ix[i] = staged_index(h.ext[i], h.image_blocks, ds, h.buf_bytes);
    std::vector<uint8_t> rows, P, st_own;
    for (size_t start = 0; start < h.n;) {
        const size_t end = run_end(ix.data(), h.n, start, blocks, max_run);
        const size_t m = end - start;
        const uint32_t* rix = ix.data() + start;
        const ppfs_ecc_extent* ex = h.ext + start;
        if (rows.size() < m * raw)
            rows.resize(m * raw);
        if (P.size() < m * ds)
            P.resize(m * ds);
        uint8_t* st = h.status ? h.status + start : nullptr;
        if (!st) {
            st_own.resize(std::max(st_own.size(), m));
            st = st_own.data();
        }
        uint8_t* Pp = ds ? P.data() : nullptr;
        gather_rows_cpu(h.image, blocks, rix, m, raw, rows.data());
        if (!h.write) {
            if ((r = ppfs_ecc_decode_host(c, rows.data(), Pp, st, m, wb ? 1 : 0, nullptr)))
                return r;
            if (ds && h.buf_bytes)
                pack_cpu(P.data(), ds, ex, rix, st, m, h.out);
        } else {
            if (ds && (r = ppfs_ecc_decode_host(c, rows.data(), Pp, nullptr, m, 0, nullptr)))
                return r;
            if (ds && h.buf_bytes)
                overlay_cpu(h.in, ex, rix, m, P.data(), ds);
            if ((r = ppfs_ecc_write_host(c, Pp, rows.data(), st, m)))
                return r;
        }
        for (uint32_t i : copy_back_list(h.write ? OP_WRITE : OP_DECODE, wb, rix, m, blocks, st))
            std::memcpy(h.image + (size_t)rix[i] * raw, rows.data() + (size_t)i * raw, raw);
        mark_out_of_range(rix, m, blocks, h.status ? st : nullptr, nullptr, 0);
        start = end;
    }
    return 0;
}

} // namespace

extern "C" int ppfs_ecc_read_extents_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_extent* ext,
    size_t n, uint8_t* out, size_t out_bytes, uint8_t* status, int write_back)
{
    return host_extents_run(c, HostExtents { false, nullptr, out, out_bytes, image, image_blocks, ext, n, status, write_back });
}

extern "C" int ppfs_ecc_write_extents_host(ppfs_ecc_ctx* c, const uint8_t* in, size_t in_bytes, uint8_t* image,
    size_t image_blocks, const ppfs_ecc_extent* ext, size_t n, uint8_t* status)
{
    return host_extents_run(c, HostExtents { true, in, nullptr, in_bytes, image, image_blocks, ext, n, status, 0 });
}
