// file_path.cpp -- the read-only file walk of the ppfs_ecc C ABI (include/ppfs_ecc.h): ppfs_ecc_file_span,
// ppfs_ecc_file_tree_blocks, ppfs_ecc_file_blocks_* (a range of a file's blocks resolved through its
// index-block tree) and ppfs_ecc_read_file_* (FileIO::readFile, lib/file_io/src/file_io.cpp:12-44, whose
// BlockIndexIterator, :186-463, reads the singly, doubly and trebly indirect index blocks one readBlock
// at a time, each depending on the one before).
//
// The index blocks are ordinary blocks of the image, the tree is at most three levels deep, and the number
// of index blocks at each level follows from the range alone (file_plan.hpp).  So:
//   tree    per level A, B, C: expand the level's pointers out of its parents' decoded payloads
//           (file_walk.hip), list-decode them (ppfs_ecc_decode_list_*: payloads and statuses into the
//           scratch, write-back), merge the inherited statuses over the decode's, tally
//   blocks  per piece of fileplan::PIECE_BLOCKS file blocks: expand the data pointers and path statuses
//   read    per piece: the same, the extents in closed form, ppfs_ecc_read_extents_*, then path status
//           over read status, the zero fill under a failed index block and the tally
//   write   ppfs_ecc_write_file_* (FileIO::writeFile over an existing range, file_io.cpp:46-104): per piece the
//           same expansion and extents, pos pointing into the caller's bytes, ppfs_ecc_write_extents_*, then
//           path status over write status, the tally and `written`; no payload byte is filled in
// The device forms queue all of it on the caller's stream and read nothing back; their scratch is the
// context's scrub scratch (scrub_path.cpp), so no call allocates or frees on the caller's stream.  The
// host forms run the same plan on the CPU around the *_host list and extent calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "file_plan.hpp"
#include "kernels.hpp"
#include "list_call.hpp"

using namespace ppfs;
using namespace ppfs::fileplan;

static_assert(sizeof(ppfs_ecc_file) == 64, "ppfs_ecc_file is sixteen dwords");
static_assert(sizeof(ppfs_ecc_file_counts) == 64, "ppfs_ecc_file_counts is eight 64-bit words");

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t blocks_seen(size_t image_blocks) { return std::min<size_t>(image_blocks, NO_BLOCK); } // NO_BLOCK names no block

// The checks of a walk over the file blocks [first, first + n) that need no GPU
// (image_needed: not for the pure arithmetic of ppfs_ecc_file_tree_blocks)
int walk_args(const ppfs_ecc_ctx* c, const void* image, bool image_needed, const ppfs_ecc_file* file, uint64_t first, uint64_t n,
    const void* index, const void* tree_index, const void* counts, const char* who)
{
    if (!c || !file)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null context or file record").c_str());
    if ((((uintptr_t)index | (uintptr_t)tree_index) & 3u) || ((uintptr_t)counts & 7u))
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": index arrays are 4-byte, the counts record 8-byte aligned").c_str());
    if (n == 0)
        return 0;
    if (image_needed && !image)
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": null image").c_str());
    if (first + n < first || first + n > occupied(file->file_size, c->data) || first + n > capacity(c->data))
        return fail(PPFS_ECC_EINVAL, (std::string(who) + ": blocks at or past the file's end or the tree's capacity").c_str());
    return 0;
}

// The checks of readFile(offset, nbytes): the span, then the walk's
int read_args(const ppfs_ecc_ctx* c, const void* image, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes,
    const void* out, uint64_t out_bytes, const void* counts, Span& sp)
{
    sp = Span { 0, 0, 0, true };
    if (!c || !file)
        return fail(PPFS_ECC_EINVAL, "read file: null context or file record");
    sp = span(file->file_size, c->data, offset, nbytes);
    if (!sp.ok)
        return fail(PPFS_ECC_EINVAL, "read file: offset at or past the file's end");
    if (c->data > 0xFFFFu)
        return fail(PPFS_ECC_EINVAL, "read file: payloads past 65,535 bytes do not fit an extent");
    int r = walk_args(c, image, true, file, sp.first, sp.count, nullptr, nullptr, counts, "read file");
    if (r || sp.count == 0)
        return r;
    if (!out || out_bytes < sp.bytes)
        return fail(PPFS_ECC_EINVAL, "read file: the out buffer is null or shorter than the bytes to deliver");
    return 0;
}

// The checks of an in-place writeFile(offset, nbytes): the range must lie inside the file (nothing is clamped,
// nothing grows), then the walk's
int write_args(const ppfs_ecc_ctx* c, const void* image, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes,
    const void* in, uint64_t in_bytes, const void* written, const void* counts, Span& sp)
{
    sp = Span { 0, 0, 0, true };
    if (!c || !file)
        return fail(PPFS_ECC_EINVAL, "write file: null context or file record");
    if (((uintptr_t)written | (uintptr_t)counts) & 7u)
        return fail(PPFS_ECC_EINVAL, "write file: the written word and the counts record are 8-byte aligned");
    if (nbytes == 0)
        return 0;
    if (offset + nbytes < offset || offset + nbytes > file->file_size)
        return fail(PPFS_ECC_EINVAL, "write file: the range runs past the file's end (a write does not grow the file)");
    sp = span(file->file_size, c->data, offset, nbytes);
    if (!sp.ok)
        return fail(PPFS_ECC_EINVAL, "write file: a codec without payload holds no file");
    if (c->data > 0xFFFFu)
        return fail(PPFS_ECC_EINVAL, "write file: payloads past 65,535 bytes do not fit an extent");
    const int r = walk_args(c, image, true, file, sp.first, sp.count, nullptr, nullptr, counts, "write file");
    if (r)
        return r;
    if (!in || in_bytes < sp.bytes)
        return fail(PPFS_ECC_EINVAL, "write file: the in buffer is null or shorter than the bytes to write");
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// Device side
// ------------------------------------------------------------------------------------------------------
// A call's share of the context's scrub scratch.  The tree: a pointer, a decode status, an inherited
// status and a payload per slot (fileplan::tree_slots: each level starts on a 16-entry boundary, so every
// level's payload and status pointers are 16-byte aligned and a context that decodes lists directly keeps
// doing so).  A piece of file blocks: pointer, path status, extent, read status.
struct Scratch {
    uint32_t* tidx;
    uint8_t *tst, *tinh, *tpay;
    uint32_t* idx;
    uint8_t* path;
    ppfs_ecc_extent* ext;
    uint8_t* rst;
};
size_t scratch_layout(const Tree& t, size_t ds, size_t piece, bool read, uint8_t* base, Scratch* s)
{
    const size_t slots = tree_blocks(t) ? tree_slots(t) : 0;
    const size_t o_tidx = 0, o_tst = round_up(o_tidx + slots * 4, 256), o_tinh = round_up(o_tst + slots, 256),
                 o_tpay = round_up(o_tinh + slots, 256), o_idx = round_up(o_tpay + slots * ds + 16, 256),
                 o_path = round_up(o_idx + piece * 4, 256), o_ext = round_up(o_path + piece, 256),
                 o_rst = round_up(o_ext + (read ? piece * 16 : 0), 256),
                 bytes = round_up(o_rst + (read ? piece : 0), 256); // the codecs store statuses in whole 16-byte windows
    if (s)
        *s = Scratch { (uint32_t*)(base + o_tidx), base + o_tst, base + o_tinh, base + o_tpay, (uint32_t*)(base + o_idx),
            base + o_path, (ppfs_ecc_extent*)(base + o_ext), base + o_rst };
    return bytes;
}

struct DeviceWalk {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t blocks;
    const ppfs_ecc_file* file;
    Tree tree;
    size_t ds;
    Scratch x;
    int wb;
    void* stream;
    hipStream_t s() const { return (hipStream_t)stream; }

    int expand(int level, uint64_t k0, uint64_t n, uint32_t* pointer, uint8_t* inherited) const
    {
        return check_hip(ppfs_file_expand_launch(file, &tree, level, k0, n, ds, x.tpay, x.tst, x.tinh, pointer, inherited, s()),
            "file expand");
    }
    // levels A, B, C: each index block decoded once; the caller's arrays in level order (either may be null)
    int levels(uint32_t* tree_index, uint8_t* tree_status, unsigned long long* counts) const
    {
        int r = 0;
        for (int level = LEVEL_A; level <= LEVEL_C && !r; ++level) {
            const uint64_t n = level_count(tree, level), at = slot_base(tree, level), to = entry_base(tree, level);
            if (n == 0)
                continue;
            (void)((r = expand(level, 0, n, x.tidx + at, x.tinh + at))
                || (r = ppfs_ecc_decode_list_device(c, image, blocks, x.tidx + at, n, x.tpay + at * ds, x.tst + at, wb, nullptr, stream))
                || (r = check_hip(ppfs_file_merge_launch(x.tinh + at, x.tst + at, n, tree_status ? tree_status + to : nullptr,
                                      x.tidx + at, tree_index ? tree_index + to : nullptr, nullptr, 0, 0, 0, ds, counts, SLOT_INDEX,
                                      s()),
                        "file tree merge")));
        }
        return r;
    }
};

} // namespace

extern "C" int ppfs_ecc_file_span(const ppfs_ecc_ctx* c, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes,
    uint64_t* first_block, uint64_t* nblocks, uint64_t* clamped_bytes)
{
    if (!c || !file)
        return fail(PPFS_ECC_EINVAL, "file span: null context or file record");
    const Span sp = span(file->file_size, c->data, offset, nbytes);
    if (!sp.ok)
        return fail(PPFS_ECC_EINVAL, "file span: offset at or past the file's end");
    if (sp.first + sp.count > capacity(c->data))
        return fail(PPFS_ECC_EINVAL, "file span: the range's blocks pass the tree's capacity");
    if (first_block)
        *first_block = sp.first;
    if (nblocks)
        *nblocks = sp.count;
    if (clamped_bytes)
        *clamped_bytes = sp.bytes;
    return 0;
}

extern "C" long long ppfs_ecc_file_tree_blocks(const ppfs_ecc_ctx* c, const ppfs_ecc_file* file, uint64_t first_block,
    uint64_t nblocks)
{
    const int r = walk_args(c, nullptr, false, file, first_block, nblocks, nullptr, nullptr, nullptr, "file tree blocks");
    if (r)
        return r;
    return (long long)tree_blocks(tree_of(first_block, nblocks, ipb_of(c->data)));
}

extern "C" int ppfs_ecc_file_blocks_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t first_block, uint64_t nblocks, uint32_t* d_index, uint8_t* d_path_status, uint32_t* d_tree_index,
    uint8_t* d_tree_status, ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    int r = walk_args(c, d_image, true, file, first_block, nblocks, d_index, d_tree_index, d_counts, "file blocks");
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "file calls cannot be captured into a graph (shared scratch and staging)");
    unsigned long long* counts = (unsigned long long*)d_counts;
    if (counts)
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(*d_counts), s), "file counts clear");
    if (nblocks == 0)
        return 0;
    DeviceWalk w { c, d_image, blocks_seen(image_blocks), file, tree_of(first_block, nblocks, ipb_of(c->data)), c->data, {},
        write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(nblocks, PIECE_BLOCKS);
    uint8_t* scratch = nullptr;
    if ((r = scrub_scratch(c, scratch_layout(w.tree, w.ds, piece, false, nullptr, nullptr), s, &scratch)))
        return r;
    scratch_layout(w.tree, w.ds, piece, false, scratch, &w.x);
    r = w.levels(d_tree_index, d_tree_status, counts);
    if (d_index || d_path_status || counts) {
        for (uint64_t off = 0; off < nblocks && !r; off += piece) {
            const uint64_t nb = std::min<uint64_t>(piece, nblocks - off);
            uint8_t* path = d_path_status ? d_path_status + off : w.x.path;
            (void)((r = w.expand(LEVEL_DATA, off, nb, d_index ? d_index + off : nullptr, path))
                || (r = check_hip(ppfs_file_merge_launch(path, nullptr, nb, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, w.ds, counts,
                                      SLOT_FILE, s),
                        "file blocks tally")));
        }
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, nblocks, stream, "file blocks (async)");
}

extern "C" int ppfs_ecc_read_file_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, ppfs_ecc_file_counts* d_counts,
    int write_back, void* stream)
{
    Span sp;
    int r = read_args(c, d_image, file, offset, nbytes, d_out, out_bytes, d_counts, sp);
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "file calls cannot be captured into a graph (shared scratch and staging)");
    unsigned long long* counts = (unsigned long long*)d_counts;
    if (counts)
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(*d_counts), s), "file counts clear");
    if (sp.count == 0)
        return 0;
    DeviceWalk w { c, d_image, blocks_seen(image_blocks), file, tree_of(sp.first, sp.count, ipb_of(c->data)), c->data, {},
        write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(sp.count, PIECE_BLOCKS);
    const uint64_t off0 = offset % w.ds;
    uint8_t* scratch = nullptr;
    if ((r = scrub_scratch(c, scratch_layout(w.tree, w.ds, piece, true, nullptr, nullptr), s, &scratch)))
        return r;
    scratch_layout(w.tree, w.ds, piece, true, scratch, &w.x);
    r = w.levels(nullptr, nullptr, counts);
    for (uint64_t off = 0; off < sp.count && !r; off += piece) {
        const uint64_t nb = std::min<uint64_t>(piece, sp.count - off);
        (void)((r = w.expand(LEVEL_DATA, off, nb, w.x.idx, w.x.path))
            || (r = check_hip(ppfs_file_extents_launch(w.x.idx, w.x.path, off, nb, off0, sp.bytes, w.ds, w.x.ext, s), "file extents"))
            || (r = ppfs_ecc_read_extents_device(c, d_image, image_blocks, w.x.ext, nb, d_out, sp.bytes, w.x.rst, w.wb, stream))
            || (r = check_hip(ppfs_file_merge_launch(w.x.path, w.x.rst, nb, d_status ? d_status + off : nullptr, nullptr, nullptr,
                                  d_out, off, off0, sp.bytes, w.ds, counts, SLOT_FILE, s),
                    "file read merge")));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, sp.count, stream, "read file (async)");
}

// FileIO::writeFile over an existing range (file_io.cpp:46-104): the read's walk and extents with pos pointing
// into `in`, ppfs_ecc_write_extents_device, then path status over write status and `written`
extern "C" int ppfs_ecc_write_file_device(ppfs_ecc_ctx* c, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* d_status, uint64_t* d_written,
    ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Span sp;
    int r = write_args(c, d_image, file, offset, nbytes, d_in, in_bytes, d_written, d_counts, sp);
    if (r)
        return r;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "file calls cannot be captured into a graph (shared scratch and staging)");
    unsigned long long *counts = (unsigned long long*)d_counts, *written = (unsigned long long*)d_written;
    if (counts)
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(*d_counts), s), "file counts clear");
    if ((r = check_hip(ppfs_file_written_init_launch(written, sp.bytes, s), "file written init")) || sp.count == 0)
        return r;
    DeviceWalk w { c, d_image, blocks_seen(image_blocks), file, tree_of(sp.first, sp.count, ipb_of(c->data)), c->data, {},
        write_back ? 1 : 0, stream };
    const size_t piece = std::min<uint64_t>(sp.count, PIECE_BLOCKS);
    const uint64_t off0 = offset % w.ds;
    uint8_t* scratch = nullptr;
    if ((r = scrub_scratch(c, scratch_layout(w.tree, w.ds, piece, true, nullptr, nullptr), s, &scratch)))
        return r;
    scratch_layout(w.tree, w.ds, piece, true, scratch, &w.x);
    r = w.levels(nullptr, nullptr, counts);
    for (uint64_t off = 0; off < sp.count && !r; off += piece) {
        const uint64_t nb = std::min<uint64_t>(piece, sp.count - off);
        (void)((r = w.expand(LEVEL_DATA, off, nb, w.x.idx, w.x.path))
            || (r = check_hip(ppfs_file_extents_launch(w.x.idx, w.x.path, off, nb, off0, sp.bytes, w.ds, w.x.ext, s), "file extents"))
            || (r = ppfs_ecc_write_extents_device(c, d_in, sp.bytes, d_image, image_blocks, w.x.ext, nb, w.x.rst, stream))
            || (r = check_hip(ppfs_file_write_merge_launch(w.x.path, w.x.rst, nb, d_status ? d_status + off : nullptr, off, off0,
                                  sp.bytes, w.ds, written, counts, s),
                    "file write merge")));
    }
    scrub_scratch_used(c, s);
    return call_queued(c, r, sp.count, stream, "write file (async)");
}

// ------------------------------------------------------------------------------------------------------
// Host side: the same plan on the CPU
// ------------------------------------------------------------------------------------------------------
namespace {

struct HostSrc {
    const ppfs_ecc_file* file;
    const uint8_t *payload, *st, *inh;
    uint32_t inode(uint32_t dw) const { return ((const uint32_t*)file)[dw]; }
    uint32_t status(uint64_t p) const { return st[p]; }
    uint32_t inherited(uint64_t p) const { return inh[p]; }
    uint32_t payload_byte(uint64_t at) const { return payload[at]; }
};

void count_host(ppfs_ecc_file_counts* counts, uint32_t st, int slot0)
{
    const int slot = count_slot(st);
    if (counts && slot >= 0)
        ++(&counts->ok)[slot0 + slot];
}

struct HostWalk {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t blocks;
    const ppfs_ecc_file* file;
    Tree tree;
    size_t ds;
    int wb;
    std::vector<uint32_t> tidx;
    std::vector<uint8_t> tst, tinh, tpay;

    HostSrc src() const { return HostSrc { file, tpay.data(), tst.data(), tinh.data() }; }
    int levels(uint32_t* tree_index, uint8_t* tree_status, ppfs_ecc_file_counts* counts)
    {
        const size_t slots = tree_blocks(tree) ? tree_slots(tree) : 0;
        tidx.assign(slots, NO_BLOCK);
        tst.assign(slots, 0);
        tinh.assign(slots, 0);
        tpay.assign(slots * ds, 0);
        for (int level = LEVEL_A; level <= LEVEL_C; ++level) {
            const uint64_t n = level_count(tree, level), at = slot_base(tree, level), to = entry_base(tree, level);
            if (n == 0)
                continue;
            for (uint64_t k = 0; k < n; ++k) {
                const Expanded e = expand(tree, level, k, ds, src());
                tidx[at + k] = e.pointer;
                tinh[at + k] = e.inherited;
            }
            const int r = ppfs_ecc_decode_list_host(c, image, blocks, tidx.data() + at, n, tpay.data() + at * ds, tst.data() + at, wb,
                nullptr);
            if (r)
                return r;
            for (uint64_t k = 0; k < n; ++k) {
                const uint8_t st = tinh[at + k] ? tinh[at + k] : tst[at + k];
                if (tree_index)
                    tree_index[to + k] = tidx[at + k];
                if (tree_status)
                    tree_status[to + k] = st;
                count_host(counts, st, SLOT_INDEX);
            }
        }
        return 0;
    }
};

} // namespace

extern "C" int ppfs_ecc_file_blocks_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t first_block, uint64_t nblocks, uint32_t* index, uint8_t* path_status, uint32_t* tree_index, uint8_t* tree_status,
    ppfs_ecc_file_counts* counts, int write_back)
{
    int r = walk_args(c, image, true, file, first_block, nblocks, index, tree_index, counts, "file blocks (host)");
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (nblocks == 0)
        return 0;
    HostWalk w { c, image, blocks_seen(image_blocks), file, tree_of(first_block, nblocks, ipb_of(c->data)), c->data, write_back ? 1 : 0,
        {}, {}, {}, {} };
    if ((r = w.levels(tree_index, tree_status, counts)))
        return r;
    const HostSrc src = w.src();
    for (uint64_t k = 0; k < nblocks; ++k) {
        const Expanded e = expand(w.tree, LEVEL_DATA, k, w.ds, src);
        if (index)
            index[k] = e.pointer;
        if (path_status)
            path_status[k] = e.inherited;
        count_host(counts, e.inherited, SLOT_FILE);
    }
    return 0;
}

extern "C" int ppfs_ecc_read_file_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* out, size_t out_bytes, uint8_t* status, ppfs_ecc_file_counts* counts, int write_back)
{
    Span sp;
    int r = read_args(c, image, file, offset, nbytes, out, out_bytes, counts, sp);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (sp.count == 0)
        return 0;
    HostWalk w { c, image, blocks_seen(image_blocks), file, tree_of(sp.first, sp.count, ipb_of(c->data)), c->data, write_back ? 1 : 0,
        {}, {}, {}, {} };
    if ((r = w.levels(nullptr, nullptr, counts)))
        return r;
    const HostSrc src = w.src();
    const uint64_t off0 = offset % w.ds;
    std::vector<ppfs_ecc_extent> ext(sp.count);
    std::vector<uint8_t> path(sp.count), rst(sp.count);
    for (uint64_t k = 0; k < sp.count; ++k) {
        const Expanded e = expand(w.tree, LEVEL_DATA, k, w.ds, src);
        const Extent x = extent_of(k, off0, sp.bytes, w.ds);
        path[k] = e.inherited;
        ext[k] = ppfs_ecc_extent { x.pos, e.inherited ? NO_BLOCK : e.pointer, (uint16_t)x.offset, (uint16_t)x.length };
    }
    if ((r = ppfs_ecc_read_extents_host(c, image, image_blocks, ext.data(), sp.count, out, sp.bytes, rst.data(), w.wb)))
        return r;
    for (uint64_t k = 0; k < sp.count; ++k) {
        const uint8_t st = path[k] ? path[k] : rst[k];
        if (status)
            status[k] = st;
        if (path[k] == STATUS_FAILED)
            std::memset(out + ext[k].pos, 0, ext[k].length);
        count_host(counts, st, SLOT_FILE);
    }
    return 0;
}

extern "C" int ppfs_ecc_write_file_host(ppfs_ecc_ctx* c, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* status, uint64_t* written, ppfs_ecc_file_counts* counts,
    int write_back)
{
    Span sp;
    int r = write_args(c, image, file, offset, nbytes, in, in_bytes, written, counts, sp);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (written)
        *written = sp.bytes;
    if (sp.count == 0)
        return 0;
    HostWalk w { c, image, blocks_seen(image_blocks), file, tree_of(sp.first, sp.count, ipb_of(c->data)), c->data, write_back ? 1 : 0,
        {}, {}, {}, {} };
    if ((r = w.levels(nullptr, nullptr, counts)))
        return r;
    const HostSrc src = w.src();
    const uint64_t off0 = offset % w.ds;
    std::vector<ppfs_ecc_extent> ext(sp.count);
    std::vector<uint8_t> path(sp.count), wst(sp.count);
    for (uint64_t k = 0; k < sp.count; ++k) {
        const Expanded e = expand(w.tree, LEVEL_DATA, k, w.ds, src);
        const Extent x = extent_of(k, off0, sp.bytes, w.ds);
        path[k] = e.inherited;
        ext[k] = ppfs_ecc_extent { x.pos, e.inherited ? NO_BLOCK : e.pointer, (uint16_t)x.offset, (uint16_t)x.length };
    }
    if ((r = ppfs_ecc_write_extents_host(c, in, sp.bytes, image, image_blocks, ext.data(), sp.count, wst.data())))
        return r;
    for (uint64_t k = sp.count; k-- > 0;) {
        const uint8_t st = path[k] ? path[k] : wst[k];
        if (status)
            status[k] = st;
        if (written && (st == STATUS_FAILED || st == STATUS_OUT))
            *written = ext[k].pos;
        count_host(counts, st, SLOT_FILE);
    }
    return 0;
}
