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
// The arithmetic and the whole per-inode rule are inode_plan.hpp's, for both forms and for reads and writes.  The
// device forms share one frame (inodes_device) that queues all of it on the caller's stream in pieces of
// inodeplan::piece_inodes(ds) inodes and reads nothing back; its scratch is the context's scrub scratch
// (scrub_path.cpp), so no call allocates or frees on the caller's stream.  The host forms run the same plan on the
// CPU, their bitmap step and epilogue shared too (host_bitmap_step, host_epilogue).
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

using namespace ppfs::inodewplan;

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the arguments the four calls share; files and meta are the read's outputs and the write's inputs
struct InodeCall {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t image_blocks;
    const ppfs_ecc_inode_table* table;
    const void* ino;
    size_t stride, n;
    const void *files, *meta;
    uint8_t *status, *piece_status;
    ppfs_ecc_inode_counts* counts;
    int wb;
};

// the checks that need no GPU
int inode_args(const InodeCall& a, bool write, const char* who)
{
    auto bad = [&](const char* what) { return fail(PPFS_ECC_EINVAL, (std::string(who) + ": " + what).c_str()); };
    if (!a.c)
        return bad("null context");
    if (!a.table)
        return bad("null inode table");
    if (a.stride < 4)
        return bad("an inode number is four bytes: the stride is at least 4");
    if (((uintptr_t)a.files & 3u) || (((uintptr_t)a.meta | (uintptr_t)a.counts) & 7u))
        return bad("the file records are 4-byte, the metadata and the counts record 8-byte aligned");
    if (a.c->data == 0 || a.c->data > 0xFFFFu)
        return bad("payloads of 0 or past 65,535 bytes do not fit an extent");
    if (a.n && (!a.image || !a.ino))
        return bad("null image or inode numbers");
    if (a.n > (size_t)-1 / a.stride)
        return bad("the inode numbers' bytes overflow");
    if (write && a.n && (!a.files || !a.meta))
        return bad("null file records or metadata");
    return 0;
}

// A piece's share of the scrub scratch, one layout for both calls: numbers, bitmap bytes and statuses, the bitmap
// extents and K extents per inode; the read's 81-byte rows and K piece statuses per inode (no bytes in a write); the
// write's status per slot and its two election tables of `cap` entries (no bytes in a read, cap = 0).  Every array is
// 256-byte aligned: the status arrays at least 16-byte, as the codecs want them
struct Scratch {
    uint32_t* ino;
    uint8_t *bm, *bst, *rows, *pst, *wst;
    ppfs_ecc_extent *bext, *text;
    uint32_t* tab;
};
size_t scratch_layout(size_t piece, uint32_t K, uint32_t cap, uint8_t* base, Scratch* s)
{
    const size_t rd = cap ? 0 : piece, wr = cap ? piece : 0;
    size_t end = 0;
    auto take = [&](size_t bytes) {
        const size_t at = end;
        end = round_up(end + bytes, 256);
        return at;
    };
    const size_t o_ino = take(piece * 4), o_bm = take(piece), o_bst = take(piece), o_rows = take(rd * INODE_BYTES), o_pst = take(rd * K),
                 o_wst = take(wr * K), o_bext = take(piece * 16), o_text = take(piece * K * 16), o_tab = take(cap ? table_bytes(cap) : 0);
    if (s)
        *s = Scratch { (uint32_t*)(base + o_ino), base + o_bm, base + o_bst, base + o_rows, base + o_pst, base + o_wst,
            (ppfs_ecc_extent*)(base + o_bext), (ppfs_ecc_extent*)(base + o_text), (uint32_t*)(base + o_tab) };
    return end;
}

// The frame of the two device forms.  A piece is piece_inodes(ds) inodes; in a write no more than one piece of the
// extent write holds the slots of, since a slot index is a row of its payload staging.  Per piece the bitmap steps,
// then steps(x, off, m, cap): what the call queues behind them for the m inodes from `off`, its result
template <class Steps>
int inodes_device(const InodeCall& a, bool write, void* stream, Steps steps)
{
    int r = inode_args(a, write, write ? "write inodes" : "read inodes");
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "inode calls cannot be captured into a graph (shared scratch and staging)");
    if (a.counts)
        HIP_TRY(hipMemsetAsync(a.counts, 0, sizeof(*a.counts), s), "inode counts clear");
    if (a.n == 0)
        return 0;
    const size_t ds = a.c->data;
    const uint32_t K = max_pieces(ds);
    const size_t most = write ? std::min<size_t>(piece_inodes(ds), std::max<size_t>(piece_of(a.c) / K, 1)) : piece_inodes(ds);
    const size_t piece = std::min(a.n, most);
    const uint32_t cap = write ? capacity(piece * K) : 0;
    (void)call_ordered(a.c, a.n, stream);
    uint8_t* base = nullptr;
    if ((r = scrub_scratch(a.c, scratch_layout(piece, K, cap, nullptr, nullptr), s, &base)))
        return r;
    Scratch x {};
    scratch_layout(piece, K, cap, base, &x);
    for (size_t off = 0; off < a.n && !r; off += piece) {
        const size_t m = std::min(piece, a.n - off);
        (void)((r = check_hip(ppfs_inode_bitmap_extents_launch((const uint8_t*)a.ino + off * a.stride, a.stride, m, a.table, ds, x.ino,
                         x.bext, s),
                    "inode bitmap extents"))
            || (a.table->check_bitmap
                && (r = ppfs_ecc_read_extents_device(a.c, a.image, a.image_blocks, x.bext, m, x.bm, m, x.bst, a.wb, stream)))
            || (r = steps(x, off, m, cap)));
    }
    scrub_scratch_used(a.c, s);
    return call_queued(a.c, r, a.n, stream, write ? "write inodes (async)" : "read inodes (async)");
}

// ---- the host forms: the same plan on the CPU ----
uint32_t load_ino(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
Table table_of(const ppfs_ecc_inode_table& t) { return Table { t.table_block, t.bitmap_block, t.total_inodes, t.check_bitmap }; }

// what the host forms share in front of their runs
int host_begin(const InodeCall& a, bool write)
{
    const int r = inode_args(a, write, write ? "write inodes (host)" : "read inodes (host)");
    if (!r && a.counts)
        *a.counts = ppfs_ecc_inode_counts {};
    return r;
}

// The bitmap step for the run of m inodes from `off`: the numbers, the bitmap bytes, their read statuses and the verdicts
struct HostRun {
    size_t off;
    std::vector<uint32_t> ino, verdict;
    std::vector<uint8_t> bm, bst;
};
int host_bitmap_step(const InodeCall& a, size_t off, size_t m, HostRun* h)
{
    const size_t ds = a.c->data;
    const Table t = table_of(*a.table);
    *h = HostRun { off, std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<uint8_t>(m, 0), std::vector<uint8_t>(m, 0) };
    for (size_t j = 0; j < m; ++j)
        h->ino[j] = load_ino((const uint8_t*)a.ino + (off + j) * a.stride);
    if (t.check_bitmap) {
        std::vector<ppfs_ecc_extent> ext(m, ppfs_ecc_extent { 0, NO_BLOCK, 0, 0 });
        for (size_t j = 0; j < m; ++j) {
            const BitByte b = bitmap_byte(t.bitmap_block, h->ino[j], ds);
            if (h->ino[j] < t.total_inodes && b.block < NO_BLOCK)
                ext[j] = ppfs_ecc_extent { j, (uint32_t)b.block, (uint16_t)b.offset, 1 };
        }
        if (int r = ppfs_ecc_read_extents_host(a.c, a.image, a.image_blocks, ext.data(), m, h->bm.data(), m, h->bst.data(), a.wb))
            return r;
    }
    for (size_t j = 0; j < m; ++j)
        h->verdict[j] = bitmap_step(t, h->ino[j], h->bm[j], h->bst[j]).verdict;
    return 0;
}
// The epilogue of inode j of the run: status, the piece_status row and the counts; piece_status(k): as inode_status's
template <class PieceStatus>
uint32_t host_epilogue(const InodeCall& a, const HostRun& h, size_t j, PieceStatus piece_status)
{
    const uint32_t K = max_pieces(a.c->data);
    const uint32_t st = inode_status(bitmap_step(table_of(*a.table), h.ino[j], h.bm[j], h.bst[j]), h.ino[j], a.c->data, K, piece_status,
        a.piece_status ? a.piece_status + (h.off + j) * (1u + K) : nullptr);
    if (a.status)
        a.status[h.off + j] = (uint8_t)st;
    const int slot = count_slot(st);
    if (a.counts && slot >= 0)
        ++(&a.counts->ok)[slot];
    return st;
}

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

// Behind the bitmap steps: the table extents, the extent read of the pieces, the merge
extern "C" int ppfs_ecc_read_inodes_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, ppfs_ecc_file* d_files, ppfs_ecc_inode_meta* d_meta, uint8_t* d_status,
    uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream)
{
    const InodeCall a { c, d_image, image_blocks, table, d_ino, ino_stride, n, d_files, d_meta, d_status, d_piece_status, d_counts,
        write_back ? 1 : 0 };
    hipStream_t s = (hipStream_t)stream;
    return inodes_device(a, false, stream, [&](const Scratch& x, size_t off, size_t m, uint32_t) {
        const size_t ds = c->data, K = max_pieces(ds);
        int r;
        (void)((r = check_hip(ppfs_inode_table_extents_launch(x.ino, x.bm, x.bst, m, table, ds, x.text, s), "inode table extents"))
            || (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, x.text, m * K, x.rows, m * INODE_BYTES, x.pst, a.wb, stream))
            || (r = check_hip(ppfs_inode_merge_launch(x.ino, x.bm, x.bst, x.rows, x.pst, m, table, ds, d_files ? d_files + off : nullptr,
                                  d_meta ? d_meta + off : nullptr, d_status ? d_status + off : nullptr,
                                  d_piece_status ? d_piece_status + off * (1u + K) : nullptr, (unsigned long long*)d_counts, s),
                    "inode merge")));
        return r;
    });
}

// The whole batch is one run: behind the bitmap step one read of all the table pieces, the row split and the epilogue
extern "C" int ppfs_ecc_read_inodes_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino_src, size_t ino_stride, size_t n, ppfs_ecc_file* files, ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back)
{
    const InodeCall a { c, image, image_blocks, table, ino_src, ino_stride, n, files, meta, status, piece_status, counts, write_back ? 1 : 0 };
    int r = host_begin(a, false);
    if (r || n == 0)
        return r;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    HostRun h;
    if ((r = host_bitmap_step(a, 0, n, &h)))
        return r;
    std::vector<uint8_t> rows(n * INODE_BYTES, 0), pst(n * K, 0);
    std::vector<ppfs_ecc_extent> ext(n * K);
    for (size_t j = 0; j < n; ++j)
        for (uint32_t k = 0; k < K; ++k)
            ext[j * K + k] = slot_extent<ppfs_ecc_extent>(slot_of(table->table_block, h.ino[j], k, h.verdict[j], ds), j);
    if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), n * K, rows.data(), n * INODE_BYTES, pst.data(), a.wb)))
        return r;
    for (size_t j = 0; j < n; ++j) {
        const uint8_t* my = pst.data() + j * K;
        const uint32_t st = host_epilogue(a, h, j, [&](uint32_t k) { return (uint32_t)my[k]; });
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
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// The inode writes: InodeManager::update (inode_manager.cpp:142-159) over a batch.  The bitmap steps are the reads';
// then the grouping step of inode_wplan.hpp turns the batch's pieces, several per table block, into one extent per
// distinct block, and ONE extent write (extent_path.cpp write_extents_pieces) checks those blocks, lets the overlay
// kernel put every winning entry's bytes onto the old payloads and encodes them again.
// ---------------------------------------------------------------------------------------
extern "C" int ppfs_ecc_write_inodes_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* d_ino, size_t ino_stride, size_t n, const ppfs_ecc_file* d_files, const ppfs_ecc_inode_meta* d_meta, uint8_t* d_status,
    uint8_t* d_piece_status, ppfs_ecc_inode_counts* d_counts, int write_back, void* stream)
{
    const InodeCall a { c, d_image, image_blocks, table, d_ino, ino_stride, n, d_files, d_meta, d_status, d_piece_status, d_counts,
        write_back ? 1 : 0 };
    hipStream_t s = (hipStream_t)stream;
    return inodes_device(a, true, stream, [&](const Scratch& x, size_t off, size_t m, uint32_t cap) {
        const size_t ds = c->data, K = max_pieces(ds);
        const ExtOverlay overlay = [&](const ExtPiece& p) {
            return p.first == 0 && p.nb == m * K
                ? check_hip(ppfs_inode_overlay_launch(x.ino, x.bm, x.bst, m, table, ds, x.tab, cap, d_files + off, d_meta + off, p.idx, p.P,
                                p.P_cap, p.s),
                      "inode overlay")
                : fail(PPFS_ECC_EINVAL, "write inodes: a piece's slots exceed one extent piece");
        };
        int r;
        (void)((r = check_hip(hipMemsetAsync(x.tab, 0xFF, table_bytes(cap), s), "inode election clear"))
            || (r = check_hip(ppfs_inode_elect_launch(x.ino, x.bm, x.bst, m, table, ds, x.tab, cap, x.text, s), "inode elect"))
            || (r = write_extents_pieces(c, d_image, image_blocks, x.text, m * K, 0, x.wst, stream, overlay, "write inodes: extents (async)"))
            || (r = check_hip(ppfs_inode_write_status_launch(x.ino, x.bm, x.bst, x.wst, m, table, ds, x.tab, cap,
                                  d_status ? d_status + off : nullptr, d_piece_status ? d_piece_status + off * (1u + K) : nullptr,
                                  (unsigned long long*)d_counts, s),
                    "inode write status")));
        return r;
    });
}

// The groups found with an ordinary map: behind the bitmap step one read of the blocks' hulls (the bytes between two
// batch inodes stay the old ones), one write of the hulls, the epilogue
extern "C" int ppfs_ecc_write_inodes_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_inode_table* table,
    const void* ino_src, size_t ino_stride, size_t n, const ppfs_ecc_file* files, const ppfs_ecc_inode_meta* meta, uint8_t* status,
    uint8_t* piece_status, ppfs_ecc_inode_counts* counts, int write_back)
{
    const InodeCall a { c, image, image_blocks, table, ino_src, ino_stride, n, files, meta, status, piece_status, counts, write_back ? 1 : 0 };
    int r = host_begin(a, true);
    if (r || n == 0)
        return r;
    const size_t ds = c->data;
    const uint32_t K = max_pieces(ds);
    const size_t chunk = (size_t)1 << 20; // slot indices stay 32-bit; chunks in batch order are the loop in batch order
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = std::min(chunk, n - off);
        HostRun h;
        if ((r = host_bitmap_step(a, off, m, &h)))
            return r;
        const std::vector<uint32_t>&ino = h.ino, &verdict = h.verdict;
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
        for (size_t j = 0; j < m; ++j)
            host_epilogue(a, h, j, [&](uint32_t k) -> uint32_t {
                const Slot sl = slot_of(table->table_block, ino[j], k, verdict[j], ds);
                if (!sl.takes_part)
                    return ST_OUT;
                const size_t g = plan.group.at(sl.block);
                return seen_status(gst[g], (uint32_t)(j * K + k), plan.groups[g].owner);
            });
    }
    return 0;
}
