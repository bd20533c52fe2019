// extent_path.cpp -- the byte-extent entry points of the ppfs_ecc C ABI (include/ppfs_ecc.h): reads and
// writes of "these n byte ranges of those blocks", a batch of readBlock({block, offset}, length) /
// writeBlock(bytes, {block, offset}) calls (rs_block_device.cpp:25-93, crc_block_device.cpp:69-122,
// hamming_block_device.cpp:111-162, parity_block_device.cpp:31-88) -- what FileIO::readFile / writeFile
// (lib/file_io/src/file_io.cpp:24-42, 50-88) issue for a file range that starts and ends mid-block, and
// what the inode table, bitmap and directory code issue for their few bytes.
//
// Device forms: the block-list calls' pipeline with its kernels and codecs unchanged (list_path.cpp:
// gather the listed rows into the context's staging, run the codec there, scatter the changed rows
// back), in pieces of the same size, plus a second staging for the decoded payloads P of a piece and
// the staged index of its entries.  An entry that is invalid is staged as index 0xFFFFFFFF, which the
// gather, scatter and range-mark kernels already treat as out of range.
//   read   index -> gather -> decode(rows -> P, status, write_back) -> scatter (status 1) -> pack P into
//          the caller's buffer -> range marks
//   write  index -> gather -> decode(rows -> P) -> overlay the caller's bytes onto P ->
//          write(P, rows, status) -> scatter (status other than 5) -> range marks
// A context that decodes lists directly (ctx.hpp list_direct; RS(255, 255-2t), 2t <= 8) reads a piece as
//   read   index -> list decode(image, index -> P, status, write_back) -> pack P
// one kernel for the gather, decode, scatter and range marks: the staged index 0xFFFFFFFF of an invalid
// entry comes out of it as status 9 and a zero payload, and writes it as
//   write  index -> list decode(image, index -> P, status; nothing written back) -> overlay ->
//          list encode(P -> image, rs_wg_encode_list_kernel)
// where an invalid entry's codeword is stored nowhere.  P, the piece size and list_ev stay.
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

int extent_args(ppfs_ecc_ctx* c, const void* image, size_t image_blocks, const void* ext, size_t n, const void* buf,
    size_t buf_bytes, const char* what)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, what);
    if (n && (!ext || ((uintptr_t)ext & 7u) || (image_blocks && !image) || (buf_bytes && !buf)))
        return fail(PPFS_ECC_EINVAL, what);
    return 0;
}

// What the pieces of one device call work with
struct Pieces {
    ppfs_ecc_ctx* c;
    size_t piece, blocks; // entries per piece; image blocks as the kernels see them
    uint8_t *rows, *P, *own_status;
    uint32_t* idx;
    size_t P_cap;
    explicit Pieces(ppfs_ecc_ctx* ctx, size_t image_blocks)
        : c(ctx)
        , piece(piece_of(ctx))
        , blocks(image_blocks_seen(image_blocks))
        , rows(ctx->d_list)
        , P(ctx->d_ext)
        , own_status(ctx->d_list + ctx->list_status_off)
        , idx((uint32_t*)(ctx->d_ext + ctx->ext_index_off))
        , P_cap(ctx->ext_index_off)
    {
    }
    // the codecs want a 16-byte aligned status array (RS, Hamming): the caller's where it is, else the
    // context's own, copied out afterwards
    uint8_t* status_for(uint8_t* d_status, size_t off) const
    {
        return d_status && (((uintptr_t)d_status & 15u) == 0) ? d_status + off : own_status;
    }
    // marks: the range marks are still to be made (the direct list decode made them itself)
    int status_out(uint8_t* st, uint8_t* d_status, size_t off, uint32_t nb, hipStream_t s, bool marks = true) const
    {
        if (!d_status)
            return 0;
        if (st != d_status + off) {
            int r = check_hip(dma_async(d_status + off, st, nb, hipMemcpyDeviceToDevice, s), "extent status copy");
            if (r)
                return r;
        }
        if (!marks)
            return 0;
        return check_hip(ppfs_list_oob_launch(idx, nb, blocks, d_status + off, nullptr, 0, s), "extent range marks");
    }
};

} // namespace

extern "C" int ppfs_ecc_read_extents_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks,
    const ppfs_ecc_extent* d_ext, size_t n, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, int write_back, void* stream)
{
    int r = extent_args(c, d_image, image_blocks, d_ext, n, d_out, out_bytes, "read extents: null or misaligned argument");
    if (r || n == 0)
        return r;
    if (stream_capturing((hipStream_t)stream))
        return fail(PPFS_ECC_ENOTSUP, "extent calls cannot be captured into a graph (shared staging)");
    ListCall call { c, (hipStream_t)stream, stream, n };
    if ((r = call.begin()))
        return r;
    if (!(r = ensure_ext_stage(c))) {
        const Pieces p(c, image_blocks);
        const bool wb = write_back && has_write_back(c);
        const uint32_t raw = c->raw, ds = c->data;
        for (size_t off = 0; off < n && !r; off += p.piece) {
            const uint32_t nb = (uint32_t)std::min(p.piece, n - off);
            const ppfs_ecc_extent* ex = d_ext + off;
            uint8_t* st = p.status_for(d_status, off); // the pack selects by status: always one
            r = check_hip(ppfs_extent_index_launch(ex, nb, p.blocks, ds, out_bytes, p.idx, call.s), "extent index");
            if (!r && c->list_direct) { // P and st are 16-byte aligned (ext_stage_layout, status_for)
                r = decode_list_direct(c, d_image, p.blocks, p.idx, nb, p.P, st, wb ? 1 : 0, nullptr, call.s);
                if (!r)
                    r = check_hip(ppfs_extent_copy_launch(0, ex, p.idx, st, nb, ds, p.P, p.P_cap, d_out, out_bytes, call.s),
                        "extent pack");
                if (!r)
                    r = p.status_out(st, d_status, off, nb, call.s, false);
                continue;
            }
            if (!r)
                r = check_hip(ppfs_gather_blocks_launch(d_image, p.blocks, p.idx, nb, raw, p.rows, call.s), "extent gather");
            if (!r)
                r = ppfs_ecc_decode_device(c, p.rows, ds ? p.P : nullptr, st, nb, wb ? 1 : 0, nullptr, stream);
            if (!r && wb)
                r = check_hip(ppfs_scatter_blocks_launch(p.rows, d_image, p.blocks, p.idx, st, 1, nb, raw, call.s),
                    "extent scatter");
            if (!r)
                r = check_hip(ppfs_extent_copy_launch(0, ex, p.idx, st, nb, ds, p.P, p.P_cap, d_out, out_bytes, call.s),
                    "extent pack");
            if (!r)
                r = p.status_out(st, d_status, off, nb, call.s);
        }
    }
    return call.end(r, "read extents (async)");
}

extern "C" int ppfs_ecc_write_extents_device(ppfs_ecc_ctx* c, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_extent* d_ext, size_t n, uint8_t* d_status, void* stream)
{
    int r = extent_args(c, d_image, image_blocks, d_ext, n, d_in, in_bytes, "write extents: null or misaligned argument");
    if (r || n == 0)
        return r;
    if (stream_capturing((hipStream_t)stream))
        return fail(PPFS_ECC_ENOTSUP, "extent calls cannot be captured into a graph (shared staging)");
    ListCall call { c, (hipStream_t)stream, stream, n };
    if ((r = call.begin()))
        return r;
    if (!(r = ensure_ext_stage(c))) {
        const Pieces p(c, image_blocks);
        const uint32_t raw = c->raw, ds = c->data;
        for (size_t off = 0; off < n && !r; off += p.piece) {
            const uint32_t nb = (uint32_t)std::min(p.piece, n - off);
            const ppfs_ecc_extent* ex = d_ext + off;
            uint8_t* st = p.status_for(d_status, off); // the scatter selects by status: always one
            r = check_hip(ppfs_extent_index_launch(ex, nb, p.blocks, ds, in_bytes, p.idx, call.s), "extent index");
            if (!r && c->list_direct) { // P and st are 16-byte aligned (ext_stage_layout, status_for)
                // the old payloads and statuses (9 and zeros for an invalid entry) without touching the
                // image, the caller's bytes over them, the new codewords stored in place
                r = decode_list_direct(c, d_image, p.blocks, p.idx, nb, p.P, st, 0, nullptr, call.s);
                if (!r)
                    r = check_hip(ppfs_extent_copy_launch(1, ex, p.idx, nullptr, nb, ds, p.P, p.P_cap,
                                      const_cast<uint8_t*>(d_in), in_bytes, call.s),
                        "extent overlay");
                if (!r)
                    r = encode_list_direct(c, p.P, d_image, p.blocks, p.idx, nb, call.s);
                if (!r)
                    r = p.status_out(st, d_status, off, nb, call.s, false);
                continue;
            }
            if (!r)
                r = check_hip(ppfs_gather_blocks_launch(d_image, p.blocks, p.idx, nb, raw, p.rows, call.s), "extent gather");
            // the old payloads: where the old block fails its check (status 5 below) the row is not
            // scattered and what P holds for it does not matter
            if (!r && ds)
                r = ppfs_ecc_decode_device(c, p.rows, p.P, nullptr, nb, 0, nullptr, stream);
            if (!r) // the kernel only reads the caller's bytes
                r = check_hip(ppfs_extent_copy_launch(1, ex, p.idx, nullptr, nb, ds, p.P, p.P_cap, const_cast<uint8_t*>(d_in),
                                  in_bytes, call.s),
                    "extent overlay");
            if (!r)
                r = ppfs_ecc_write_device(c, ds ? p.P : nullptr, p.rows, st, nb, stream);
            if (!r)
                r = check_hip(ppfs_scatter_blocks_launch(p.rows, d_image, p.blocks, p.idx, st, 2, nb, raw, call.s),
                    "extent scatter");
            if (!r)
                r = p.status_out(st, d_status, off, nb, call.s);
        }
    }
    return call.end(r, "write extents (async)");
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
    int r = extent_args(c, h.image, h.image_blocks, h.ext, h.n, h.write ? h.in : h.out, h.buf_bytes,
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
