// file_path.cpp -- the single-file entry points of the file walk of the ppfs_ecc C ABI (include/ppfs_ecc.h):
// ppfs_ecc_file_span, ppfs_ecc_file_tree_blocks, ppfs_ecc_file_blocks_* (a range of a file's blocks resolved through
// its index-block tree), ppfs_ecc_read_file_* (FileIO::readFile, lib/file_io/src/file_io.cpp:12-44, whose
// BlockIndexIterator, :186-463, reads the singly, doubly and trebly indirect index blocks one readBlock at a time,
// each depending on the one before) and ppfs_ecc_write_file_* (FileIO::writeFile over an existing range,
// file_io.cpp:46-104).
//
// Each checks its arguments, builds the plan of a batch of one file (filesplan::build_one: a fixed record on the
// stack, no heap allocation), clears the counts and runs the walk of files_path.cpp over it (file_call.hpp): the
// same kernels and the same launches as a batch, with the file's record in the kernel arguments in place of the
// batch's tables, so nothing is uploaded.
#include <hip/hip_runtime.h>

#include <string>

#include "ctx.hpp"
#include "file_call.hpp"
#include "kernels.hpp"

using namespace ppfs;
using namespace ppfs::fileplan;
using filesplan::OnePlan;

static_assert(sizeof(ppfs_ecc_file) == 64, "ppfs_ecc_file is sixteen dwords");
static_assert(sizeof(ppfs_ecc_file_counts) == 64, "ppfs_ecc_file_counts is eight 64-bit words");

namespace {

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

// what the device forms do before the walk: refuse a capture, clear the counts
int device_begin(hipStream_t s, ppfs_ecc_file_counts* d_counts)
{
    if (stream_capturing(s))
        return fail(PPFS_ECC_ENOTSUP, "file calls cannot be captured into a graph (shared scratch and staging)");
    if (d_counts)
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s), "file counts clear");
    return 0;
}

// the call over the file blocks [first, first + count) of one file: `bytes` bytes from byte `offset` of the file
FileCall one_file(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file, const Span& sp, uint64_t offset,
    OnePlan& plan, FileMode mode, int write_back, ppfs_ecc_file_counts* counts)
{
    filesplan::build_one((const uint32_t*)file, sp.first, sp.count, offset % c->data, sp.bytes, c->data, plan);
    FileCall a { c, image, image_blocks, plan.view(), mode, write_back ? 1 : 0 };
    a.counts = counts;
    return a;
}
// ... and a walk's: whole blocks
FileCall one_file_blocks(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file, uint64_t first, uint64_t n,
    OnePlan& plan, int write_back, uint32_t* index, uint8_t* path_status, uint32_t* tree_index, uint8_t* tree_status,
    ppfs_ecc_file_counts* counts)
{
    FileCall a = one_file(c, image, image_blocks, file, Span { first, n, n * c->data, true }, 0, plan, FileMode::blocks, write_back, counts);
    a.index = index;
    a.path_status = path_status;
    a.tree_index = tree_index;
    a.tree_status = tree_status;
    return a;
}

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
    if (r || (r = device_begin((hipStream_t)stream, d_counts)) || nblocks == 0)
        return r;
    OnePlan plan;
    return file_call_device(one_file_blocks(c, d_image, image_blocks, file, first_block, nblocks, plan, write_back, d_index,
                                d_path_status, d_tree_index, d_tree_status, d_counts),
        stream, "file blocks (async)");
}

extern "C" int ppfs_ecc_read_file_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* d_out, size_t out_bytes, uint8_t* d_status, ppfs_ecc_file_counts* d_counts,
    int write_back, void* stream)
{
    Span sp;
    int r = read_args(c, d_image, file, offset, nbytes, d_out, out_bytes, d_counts, sp);
    if (r || (r = device_begin((hipStream_t)stream, d_counts)) || sp.count == 0)
        return r;
    OnePlan plan;
    FileCall a = one_file(c, d_image, image_blocks, file, sp, offset, plan, FileMode::read, write_back, d_counts);
    a.out = d_out;
    a.status = d_status;
    return file_call_device(a, stream, "read file (async)");
}

extern "C" int ppfs_ecc_write_file_device(ppfs_ecc_ctx* c, const uint8_t* d_in, size_t in_bytes, uint8_t* d_image,
    size_t image_blocks, const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* d_status, uint64_t* d_written,
    ppfs_ecc_file_counts* d_counts, int write_back, void* stream)
{
    Span sp;
    int r = write_args(c, d_image, file, offset, nbytes, d_in, in_bytes, d_written, d_counts, sp);
    if (r || (r = device_begin((hipStream_t)stream, d_counts)))
        return r;
    if (sp.count == 0) { // an empty range: nothing is written, of nothing
        const filesplan::OneRec none {};
        const ppfs_files_owner who { nullptr, 0, nullptr, 0, &none };
        return check_hip(ppfs_files_written_init_launch(&who, (unsigned long long*)d_written, (hipStream_t)stream), "file written init");
    }
    OnePlan plan;
    FileCall a = one_file(c, d_image, image_blocks, file, sp, offset, plan, FileMode::write, write_back, d_counts);
    a.in = d_in;
    a.status = d_status;
    a.written = d_written;
    return file_call_device(a, stream, "write file (async)");
}

extern "C" int ppfs_ecc_file_blocks_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t first_block, uint64_t nblocks, uint32_t* index, uint8_t* path_status, uint32_t* tree_index, uint8_t* tree_status,
    ppfs_ecc_file_counts* counts, int write_back)
{
    const int r = walk_args(c, image, true, file, first_block, nblocks, index, tree_index, counts, "file blocks (host)");
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (nblocks == 0)
        return 0;
    OnePlan plan;
    return file_call_host(one_file_blocks(c, image, image_blocks, file, first_block, nblocks, plan, write_back, index, path_status,
        tree_index, tree_status, counts));
}

extern "C" int ppfs_ecc_read_file_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_blocks, const ppfs_ecc_file* file,
    uint64_t offset, uint64_t nbytes, uint8_t* out, size_t out_bytes, uint8_t* status, ppfs_ecc_file_counts* counts, int write_back)
{
    Span sp;
    const int r = read_args(c, image, file, offset, nbytes, out, out_bytes, counts, sp);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (sp.count == 0)
        return 0;
    OnePlan plan;
    FileCall a = one_file(c, image, image_blocks, file, sp, offset, plan, FileMode::read, write_back, counts);
    a.out = out;
    a.status = status;
    return file_call_host(a);
}

extern "C" int ppfs_ecc_write_file_host(ppfs_ecc_ctx* c, const uint8_t* in, size_t in_bytes, uint8_t* image, size_t image_blocks,
    const ppfs_ecc_file* file, uint64_t offset, uint64_t nbytes, uint8_t* status, uint64_t* written, ppfs_ecc_file_counts* counts,
    int write_back)
{
    Span sp;
    const int r = write_args(c, image, file, offset, nbytes, in, in_bytes, written, counts, sp);
    if (r)
        return r;
    if (counts)
        *counts = ppfs_ecc_file_counts {};
    if (written)
        *written = sp.bytes;
    if (sp.count == 0)
        return 0;
    OnePlan plan;
    FileCall a = one_file(c, image, image_blocks, file, sp, offset, plan, FileMode::write, write_back, counts);
    a.in = in;
    a.status = status;
    a.written = written;
    return file_call_host(a);
}
