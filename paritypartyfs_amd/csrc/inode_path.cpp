// inode_path.cpp -- the inode calls of the ppfs_ecc C ABI (include/ppfs_ecc.h): ppfs_ecc_inode_span,
// ppfs_ecc_read_inodes_*, InodeManager::get (lib/inode_manager/src/inode_manager.cpp:127-138) over a batch of inode
// numbers of one inode table, and ppfs_ecc_write_inodes_*, InodeManager::update (:142-159) over such a batch (the
// second half of this file).
//
// Per inode the reference reads one byte of the inode bitmap (Bitmap::getBit, bitmap.cpp:87-101) and then the 81
// bytes of the packed Inode, cut at block boundaries (_readInode, :56-89).  Both are byte extents, so a batch is two
// extent reads -- all the bitmap bytes, then all the table pieces of the inodes whose bit allows it -- with the
// decisions in between taken where the bytes are:
//   bitmap extents  one extent of one byte per inode, invalid when the number is out of range or the bitmap is not
//                   checked (then the extent read is skipped altogether)
//   table extents   K(ds) extents per inode, valid for the pieces of the inodes that passed
//   merge           the status rule, the row split into the ppfs_ecc_file record and the metadata, the tally
// The arithmetic and the status rule are inode_plan.hpp's, for both forms.  The device form queues all of it on the
// caller's stream in pieces of inodeplan::piece_inodes(ds) inodes and reads nothing back; its scratch is the
// context's scrub scratch (scrub_path.cpp), so no call allocates or frees on the caller's stream.  The host form
// runs the same plan on the CPU around two ppfs_ecc_read_extents_host calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "inode_plan.hpp"
#include "inode_wplan.hpp"
#include "kernels.hpp"
#include "list_call.hpp"

using namespace ppfs;
using namespace ppfs::inodeplan;

static_assert(sizeof(ppfs_ecc_inode_table) == 16, "table layout");
static_assert(sizeof(ppfs_ecc_inode_meta) == 24, "meta layout");
static_assert(sizeof(ppfs_ecc_inode_counts) == 64, "counts layout");
static_assert(PPFS_ECC_INODE_PIECE == PIECE_INODES, "the header's piece is the plan's");

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the checks that need no GPU
int inode_args(const ppfs_ecc_ctx* c, const void* image, const ppfs_ecc_inode_table* table, const void* ino, size_t stride, size_t n,
    const void* files, const void* meta, const void* counts, const char* who)
{
    auto bad = [&](const char* what) { return fail(PPFS_ECC_EINVAL, (std::string(who) + ": " + what).c_str()); };
    if (!c)
        return bad("null context");
    if (!table)
        return bad("null inode table");
    if (stride < 4)
        return bad("an inode number is four bytes: the stride is at least 4");
    if (((uintptr_t)files & 3u) || (((uintptr_t)meta | (uintptr_t)counts) & 7u))
        return bad("the file records are 4-byte, the metadata and the counts record 8-byte aligned");
    if (c->data == 0 || c->data > 0xFFFFu)
        return bad("payloads of 0 or past 65,535 bytes do not fit an extent");
    if (n && (!image || !ino))
        return bad("null image or inode numbers");
    if (n > (size_t)-1 / stride)
        return bad("the inode numbers' bytes overflow");
    return 0;
}

// a piece's share of the scrub scratch: numbers, bitmap bytes and statuses, the 81-byte rows, K piece statuses and
// 1 + K extents per inode.  The status arrays are 16-byte aligned, as the codecs want them
struct Scratch {
    uint32_t* ino;
    uint8_t *bm, *bst, *rows, *pst;
    ppfs_ecc_extent *bext, *text;
};
size_t scratch_layout(size_t piece, uint32_t K, uint8_t* base, Scratch* s)
{
    const size_t o_bm = round_up(piece * 4, 256), o_bst = round_up(o_bm + piece, 256), o_rows = round_up(o_bst + piece, 256),
                 o_pst = round_up(o_rows + piece * INODE_BYTES, 256), o_bext = round_up(o_pst + piece * K, 256),
                 o_text = round_up(o_bext + piece * 16, 256), bytes = round_up(o_text + piece * K * 16, 256);
    if (s)
        *s = Scratch { (uint32_t*)base, base + o_bm, base + o_bst, base + o_rows, base + o_pst, (ppfs_ecc_extent*)(base + o_bext),
            (ppfs_ecc_extent*)(base + o_text) };
    return bytes;
}

uint32_t load_ino(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

const ppfs_ecc_extent kInvalid { 0, NO_BLOCK, 0, 0 };

} // namespace

extern "C" int ppfs_ecc_inode_span(const ppfs_ecc_ctx* c, const ppfs_ecc_inode_table* table, uint32_t ino, uint32_t* block,
    uint32_t* offset, uint32_t* npieces)
{
    if (!c || !table)
        return fail(PPFS_ECC_EINVAL, "inode span: null context or inode table");
    if (c->data == 0)
        return fail(PPFS_ECC_EINVAL, "inode span: the codec has no payload");
    if (ino >= table->total_inodes)
        return fail(PPFS_ECC_EINVAL, "inode span: the inode number is at or past total_inodes");
    const Piece p = piece(table->table_block, ino, 0, c->data);
    if (p.block >= NO_BLOCK)
        return fail(PPFS_ECC_EINVAL, "inode span: the inode's block is past 2^32 - 2");
    if (block)
        *block = (uint32_t)p.block;
    if (offset)
        *offset = p.offset;
    if (npieces)
        *npieces = pieces(ino, c->data);
    return 0;
}

extern "C" int ppfs_ecc_read_inodes_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, ppfs_ecc_file* d_files, ppfs_ecc_inode_meta* d_meta, uint8_t* d_status,
    uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream)
{
    int r = inode_args(c, d_image, table, d_ino, ino_stride, n, d_files, d_meta, d_counts, "read inodes");
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "inode calls cannot be captured into a graph (shared scratch and staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "inode counts clear");
    if (n == 0)
        return 0;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    const size_t piece = std::min<size_t>(n, piece_inodes(ds));
    const int wb = write_back ? 1 : 0;
    (void)call_ordered(c, n, stream);
    uint8_t* base = nullptr;
    if ((r = scrub_scratch(c, scratch_layout(piece, K, nullptr, nullptr), s, &base)))
        return r;
    Scratch x {};
    scratch_layout(piece, K, base, &x);
    const size_t W = 1u + K;
    for (size_t off = 0; off < n && !r; off += piece) {
        const size_t m = std::min(piece, n - off);
        (void)((r = check_hip(ppfs_inode_bitmap_extents_launch((const uint8_t*)d_ino + off * ino_stride, ino_stride, m, table, ds, x.ino,
                         x.bext, s),
                    "inode bitmap extents"))
            || (table->check_bitmap && (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, x.bext, m, x.bm, m, x.bst, wb, stream)))
            || (r = check_hip(ppfs_inode_table_extents_launch(x.ino, x.bm, x.bst, m, table, ds, x.text, s), "inode table extents"))
            || (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, x.text, m * K, x.rows, m * INODE_BYTES, x.pst, wb, stream))
            || (r = check_hip(ppfs_inode_merge_launch(x.ino, x.bm, x.bst, x.rows, x.pst, m, table, ds, d_files ? d_files + off : nullptr,
                                  d_meta ? d_meta + off : nullptr, d_status ? d_status + off : nullptr,
                                  d_piece_status ? d_piece_status + off * W : nullptr, (unsigned long long*)d_counts, s),
                    "inode merge")));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, n, stream, "read inodes (async)");
}

// The same plan on the CPU: the whole batch is one piece
extern "C" int ppfs_ecc_read_inodes_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino_src, size_t ino_stride, size_t n, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back)
{
    int r = inode_args(c, image, table, ino_src, ino_stride, n, files, meta, counts, "read inodes (host)");
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_inode_counts {};
    if (n == 0)
        return 0;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    const size_t W = 1u + K;
    const bool check = table->check_bitmap != 0;
    const uint64_t total = table->total_inodes;
    const int wb = write_back ? 1 : 0;
    std::vector<uint32_t> ino(n);
    std::vector<uint8_t> bm(n, 0), bst(n, 0), rows(n * INODE_BYTES, 0), pst(n * K, 0);
    std::vector<ppfs_ecc_extent> ext(n * K, kInvalid);
    for (size_t j = 0; j < n; ++j)
        ino[j] = load_ino((const uint8_t*)ino_src + j * ino_stride);
    if (check) {
        for (size_t j = 0; j < n; ++j) {
            const BitByte b = bitmap_byte(table->bitmap_block, ino[j], ds);
            if (ino[j] < total && b.block < NO_BLOCK)
                ext[j] = ppfs_ecc_extent { j, (uint32_t)b.block, (uint16_t)b.offset, 1 };
        }
        if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), n, bm.data(), n, bst.data(), wb)))
            return r;
    }
    // what steps 1 and 2 decide; a byte that was not delivered is not looked at
    auto verdict = [&](size_t j) {
        const bool seen = check && ino[j] < total && (bst[j] == ST_OK || bst[j] == ST_CORRECTED);
        return bitmap_verdict(ino[j], total, check, bst[j], seen ? bm[j] : 0u, 0x80u >> (ino[j] % 8u));
    };
    for (size_t j = 0; j < n; ++j) {
        const uint32_t np = verdict(j) == 0u ? pieces(ino[j], ds) : 0u;
        for (uint32_t k = 0; k < K; ++k) {
            ppfs_ecc_extent e = kInvalid;
            if (k < np) {
                const Piece p = piece(table->table_block, ino[j], k, ds);
                if (p.block < NO_BLOCK)
                    e = ppfs_ecc_extent { (uint64_t)INODE_BYTES * j + p.pos, (uint32_t)p.block, (uint16_t)p.offset, (uint16_t)p.length };
            }
            ext[j * K + k] = e;
        }
    }
    if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), n * K, rows.data(), n * INODE_BYTES, pst.data(), wb)))
        return r;
    for (size_t j = 0; j < n; ++j) {
        const uint32_t v = verdict(j);
        const bool bit_read = check && ino[j] < total;
        const uint32_t np = v == 0u ? pieces(ino[j], ds) : 0u;
        const uint8_t* my = pst.data() + j * K;
        const uint32_t st = v ? v : table_status(bit_read ? bst[j] : 0u, np, [&](uint32_t k) { return (uint32_t)my[k]; });
        if (status)
            status[j] = (uint8_t)st;
        if (piece_status) {
            uint8_t* ps = piece_status + j * W;
            ps[0] = bit_read ? bst[j] : (uint8_t)ST_UNUSED;
            for (uint32_t k = 0; k < K; ++k)
                ps[1u + k] = k < np ? my[k] : (uint8_t)ST_UNUSED;
        }
        const bool good = st == ST_OK || st == ST_CORRECTED;
        const uint8_t* row = rows.data() + j * INODE_BYTES;
        auto at = [&](uint32_t i) -> uint32_t { return good ? row[i] : 0u; };
        if (files) {
            uint32_t* f = (uint32_t*)(files + j);
            for (uint32_t w = 0; w < FILE_BYTES / 4u; ++w)
                f[w] = le32(at, FILE_OFF + 4u * w);
        }
        if (meta) {
            ppfs_ecc_inode_meta m {};
            m.time_creation = le64(at, 0);
            m.time_modified = le64(at, 8);
            m.type = (uint8_t)at(TYPE_OFF);
            meta[j] = m;
        }
        const int slot = count_slot(st);
        if (counts && slot >= 0)
            ++(&counts->ok)[slot];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// The inode writes: InodeManager::update (inode_manager.cpp:142-159) over a batch.  The bitmap steps are the reads';
// then the grouping step of inode_wplan.hpp turns the batch's pieces, several per table block, into one extent per
// distinct block, and ONE extent write (extent_path.cpp write_extents_pieces) checks those blocks, lets the overlay
// kernel put every winning entry's bytes onto the old payloads and encodes them again.
// ---------------------------------------------------------------------------------------
namespace {

using namespace ppfs::inodewplan;

int write_args(const void* files, const void* meta, size_t n, const char* who)
{
    if (n && (!files || !meta))
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null file records or metadata").c_str());
    return 0;
}

// a piece's share of the scrub scratch: numbers, bitmap bytes and statuses, one write status and one extent per slot,
// the bitmap extents, the two election tables
struct WScratch {
    uint32_t* ino;
    uint8_t *bm, *bst, *wst;
    ppfs_ecc_extent *bext, *text;
    uint32_t* tab;
};
size_t wscratch_layout(size_t piece, uint32_t K, uint32_t cap, uint8_t* base, WScratch* s)
{
    const size_t o_bm = round_up(piece * 4, 256), o_bst = round_up(o_bm + piece, 256), o_wst = round_up(o_bst + piece, 256),
                 o_bext = round_up(o_wst + piece * K, 256), o_text = round_up(o_bext + piece * 16, 256),
                 o_tab = round_up(o_text + piece * K * 16, 256), bytes = round_up(o_tab + table_bytes(cap), 256);
    if (s)
        *s = WScratch { (uint32_t*)base, base + o_bm, base + o_bst, base + o_wst, (ppfs_ecc_extent*)(base + o_bext),
            (ppfs_ecc_extent*)(base + o_text), (uint32_t*)(base + o_tab) };
    return bytes;
}

} // namespace

extern "C" int ppfs_ecc_write_inodes_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, const ppfs_ecc_file* d_files, const ppfs_ecc_inode_meta* d_meta, uint8_t* d_status,
    uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream)
{
    int r = inode_args(c, d_image, table, d_ino, ino_stride, n, d_files, d_meta, d_counts, "write inodes");
    if (r || (r = write_args(d_files, d_meta, n, "write inodes")))
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "inode calls cannot be captured into a graph (shared scratch and staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "inode counts clear");
    if (n == 0)
        return 0;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    // a piece's slots are one piece of the extent write: a slot index is a row of its payload staging
    const size_t piece = std::min<size_t>(n, std::min<size_t>(piece_inodes(ds), std::max<size_t>(piece_of(c) / K, 1)));
    const uint32_t cap = capacity(piece * K);
    const int wb = write_back ? 1 : 0;
    (void)call_ordered(c, n, stream);
    uint8_t* base = nullptr;
    if ((r = scrub_scratch(c, wscratch_layout(piece, K, cap, nullptr, nullptr), s, &base)))
        return r;
    WScratch x {};
    wscratch_layout(piece, K, cap, base, &x);
    const size_t W = 1u + K;
    for (size_t off = 0; off < n && !r; off += piece) {
        const size_t m = std::min(piece, n - off);
        const ExtOverlay overlay = [&](const ExtPiece& p) {
            return p.first == 0 && p.nb == m * K
                ? check_hip(ppfs_inode_overlay_launch(x.ino, x.bm, x.bst, m, table, ds, x.tab, cap, d_files + off, d_meta + off, p.idx, p.P,
                                p.P_cap, p.s),
                      "inode overlay")
                : fail(PPFS_ECC_EINVAL, "write inodes: a piece's slots exceed one extent piece");
        };
        (void)((r = check_hip(ppfs_inode_bitmap_extents_launch((const uint8_t*)d_ino + off * ino_stride, ino_stride, m, table, ds, x.ino,
                         x.bext, s),
                    "inode bitmap extents"))
            || (table->check_bitmap && (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, x.bext, m, x.bm, m, x.bst, wb, stream)))
            || (r = check_hip(hipMemsetAsync(x.tab, 0xFF, table_bytes(cap), s), "inode election clear"))
            || (r = check_hip(ppfs_inode_elect_launch(x.ino, x.bm, x.bst, m, table, ds, x.tab, cap, x.text, s), "inode elect"))
            || (r = write_extents_pieces(c, d_image, image_blocks, x.text, m * K, 0, x.wst, stream, overlay, "write inodes: extents (async)"))
            || (r = check_hip(ppfs_inode_write_status_launch(x.ino, x.bm, x.bst, x.wst, m, table, ds, x.tab, cap,
                                  d_status ? d_status + off : nullptr, d_piece_status ? d_piece_status + off * W : nullptr,
                                  (unsigned long long*)d_counts, s),
                    "inode write status")));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, n, stream, "write inodes (async)");
}

// The same plan on the CPU, the groups found with an ordinary map: one read of the bitmap bytes, one read of the
// blocks' hulls (the bytes between two batch inodes stay the old ones), one write of the hulls
extern "C" int ppfs_ecc_write_inodes_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino_src, size_t ino_stride, size_t n, const ppfs_ecc_file* files, const ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back)
{
    int r = inode_args(c, image, table, ino_src, ino_stride, n, files, meta, counts, "write inodes (host)");
    if (r || (r = write_args(files, meta, n, "write inodes (host)")))
        return r;
    if (counts)
        *counts = ppfs_ecc_inode_counts {};
    if (n == 0)
        return 0;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    const size_t W = 1u + K;
    const bool check = table->check_bitmap != 0;
    const uint64_t total = table->total_inodes;
    const int wb = write_back ? 1 : 0;
    const size_t chunk = (size_t)1 << 20; // slot indices stay 32-bit; chunks in batch order are the loop in batch order
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        std::vector<uint32_t> ino(m), verdict(m);
        std::vector<uint8_t> bm(m, 0), bst(m, 0);
        for (size_t j = 0; j < m; ++j)
            ino[j] = load_ino((const uint8_t*)ino_src + (off + j) * ino_stride);
        if (check) {
            std::vector<ppfs_ecc_extent> ext(m, kInvalid);
            for (size_t j = 0; j < m; ++j) {
                const BitByte b = bitmap_byte(table->bitmap_block, ino[j], ds);
                if (ino[j] < total && b.block < NO_BLOCK)
                    ext[j] = ppfs_ecc_extent { j, (uint32_t)b.block, (uint16_t)b.offset, 1 };
            }
            if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), m, bm.data(), m, bst.data(), wb)))
                return r;
        }
        for (size_t j = 0; j < m; ++j) {
            const bool seen = check && ino[j] < total && (bst[j] == ST_OK || bst[j] == ST_CORRECTED);
            verdict[j] = bitmap_verdict(ino[j], total, check, bst[j], seen ? bm[j] : 0u, 0x80u >> (ino[j] % 8u));
        }
        const HostPlan plan = plan_host(ino.data(), verdict.data(), m, table->table_block, ds);
        const size_t G = plan.groups.size();
        std::vector<ppfs_ecc_extent> hull(G);
        std::vector<uint8_t> gst(G, 0);
        size_t bytes = 0;
        for (size_t g = 0; g < G; ++g) {
            const Group& gr = plan.groups[g];
            hull[g] = ppfs_ecc_extent { bytes, gr.block, (uint16_t)gr.lo, (uint16_t)(gr.hi - gr.lo) };
            bytes += gr.hi - gr.lo;
        }
        std::vector<uint8_t> buf(bytes, 0);
        if (G && (r = ppfs_ecc_read_extents_host(c, image, image_blocks, hull.data(), G, buf.data(), bytes, nullptr, 0)))
            return r;
        for (size_t j = 0; j < m; ++j) {
            auto w = plan.winner.find(ino[j]);
            if (verdict[j] != 0u || w == plan.winner.end() || w->second != j)
                continue;
            const ppfs_ecc_inode_meta& mt = meta[off + j];
            const uint8_t* f = (const uint8_t*)(files + off + j);
            for (uint32_t k = 0; k < K; ++k) {
                const Slot sl = slot_of(table->table_block, ino[j], k, verdict[j], ds);
                if (!sl.takes_part)
                    continue;
                const size_t g = plan.group.at(sl.block);
                uint8_t* dst = buf.data() + hull[g].pos + (sl.offset - plan.groups[g].lo);
                for (uint32_t b = 0; b < sl.length; ++b)
                    dst[b] = (uint8_t)row_byte(mt.time_creation, mt.time_modified, mt.type, [&](uint32_t i) -> uint32_t { return f[i]; },
                        sl.pos + b);
            }
        }
        if (G && (r = ppfs_ecc_write_extents_host(c, buf.data(), bytes, image, image_blocks, hull.data(), G, gst.data())))
            return r;
        for (size_t j = 0; j < m; ++j) {
            const uint32_t v = verdict[j];
            const bool bit_read = check && ino[j] < total;
            const uint32_t np = v == 0u ? pieces(ino[j], ds) : 0u;
            auto piece_st = [&](uint32_t k) -> uint32_t {
                const Slot sl = slot_of(table->table_block, ino[j], k, v, ds);
                if (!sl.takes_part)
                    return ST_OUT;
                const size_t g = plan.group.at(sl.block);
                return seen_status(gst[g], (uint32_t)(j * K + k), plan.groups[g].owner);
            };
            const uint32_t st = v ? v : table_status(bit_read ? bst[j] : 0u, np, piece_st);
            if (status)
                status[off + j] = (uint8_t)st;
            if (piece_status) {
                uint8_t* ps = piece_status + (off + j) * W;
                ps[0] = bit_read ? bst[j] : (uint8_t)ST_UNUSED;
                for (uint32_t k = 0; k < K; ++k)
                    ps[1u + k] = k < np ? (uint8_t)piece_st(k) : (uint8_t)ST_UNUSED;
            }
            const int slot = count_slot(st);
            if (counts && slot >= 0)
                ++(&counts->ok)[slot];
        }
    }
    return 0;
}
