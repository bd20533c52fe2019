// list_call.hpp -- what the block-list calls (list_path.cpp) and the byte-extent calls
// (extent_path.cpp) share: the argument check, the frame of one device call, and the piece of listed
// rows that a call decodes, encodes or writes.  Defined in list_path.cpp.
#pragma once

#include <functional>

#include "../../include/ppfs_ecc.h"
#include "ctx.hpp"

#pragma GCC visibility push(hidden)
namespace ppfs {

size_t piece_of(ppfs_ecc_ctx* c); // blocks per piece of a staged device list / extent call

// Null context; with n entries: a null or misaligned (align: a power of two) entry array, a null image
// of image_blocks blocks, a null buffer that is needed.  Fails as PPFS_ECC_EINVAL under the caller's text.
int entry_args(const ppfs_ecc_ctx* c, const void* image, size_t image_blocks, const void* entries, unsigned align, size_t n,
    const void* buf, bool buf_needed, const char* what);

// The frame of one device call.  begin(): refuses a capturing stream (kind: "list" / "extent", the
// refusal's wording), orders the call after the last call on the stream and, when the call uses the
// context's shared staging, makes the row staging at the context's first call and waits for its
// previous user (list_ev).  end(): records list_ev again, also after a failure, and does what every
// device entry point does after its last launch.  A call without staging (a direct list call) is one
// piece and queues nothing but its codec kernels in between.
struct ListCall {
    ppfs_ecc_ctx* c;
    void* stream;
    size_t nblocks;
    const char* kind;
    bool staging;
    hipStream_t s() const { return (hipStream_t)stream; }
    size_t piece() const { return staging ? piece_of(c) : nblocks; }
    int begin();
    int end(int r, const char* what);
};

// One piece of listed rows: entry i = image row ix[i], nb entries, every operation queued on the
// caller's stream.  The one place where the two ways to reach the rows part (the table in list_path.cpp):
// staged, through a gathered copy in the context's row staging, or direct, by codec kernels that fetch
// and store the listed rows themselves.  direct is the entry point's decision; data and st are the
// piece's, 16-byte aligned when direct.
struct PieceIO {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t blocks; // image blocks as the kernels see them
    void* stream;
    bool direct;
    bool old_status_known = false; // old_payloads() left the old blocks' statuses in st: write() need not ask again

    int fetch(const uint32_t* ix, size_t nb);
    // payloads into data, statuses into st (either may be null), corrected rows back into the image when
    // wb, spill records (null: none)
    int decode(const uint32_t* ix, size_t nb, uint8_t* data, uint8_t* st, bool wb, uint8_t* spill);
    // the old payloads into P before an overlay; the image stays as it is
    int old_payloads(const uint32_t* ix, size_t nb, uint8_t* P, uint8_t* st);
    int encode(const uint32_t* ix, size_t nb, const uint8_t* data);
    // the old blocks' statuses into st (null: not wanted), then the new codewords
    int write(const uint32_t* ix, size_t nb, const uint8_t* data, uint8_t* st);
    // status 9 and a zero payload for the entries out of range, in the caller's arrays (null: none)
    int marks(const uint32_t* ix, size_t nb, uint8_t* st, uint8_t* data);

private:
    hipStream_t s() const { return (hipStream_t)stream; }
    uint8_t* rows() const { return c->d_list; }
    uint8_t* own_status() const { return c->d_list + c->list_status_off; }
};

// The write piece loop of the byte-extent calls (extent_path.cpp) with its overlay step as a parameter.  Per piece of at
// most piece_of(c) entries: index, fetch, old payloads into P, overlay(piece), write, status out, marks.  The overlay
// queues on s whatever puts the new bytes onto the decoded payloads: row i of P (stride data size, P_cap bytes in
// all) is entry first + i of the list, idx[i] its staged index (0xFFFFFFFF: invalid, the row is not written).
// ppfs_ecc_write_extents_device passes the copy of the caller's packed bytes; the inode write (inode_path.cpp) passes
// its own kernel and a buf_bytes of 0.  The caller has checked its arguments (entry_args) and n > 0.
struct ExtPiece {
    const ppfs_ecc_extent* ex;
    const uint32_t* idx;
    uint32_t nb;
    uint8_t* P;
    size_t P_cap;
    size_t first;
    hipStream_t s;
};
using ExtOverlay = std::function<int(const ExtPiece&)>;
int write_extents_pieces(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_blocks, const ppfs_ecc_extent* d_ext, size_t n,
    size_t buf_bytes, uint8_t* d_status, void* stream, const ExtOverlay& overlay, const char* what);

// The context's scrub scratch (scrub_path.cpp), which the scrubs of named blocks and the file walk
// (files_path.cpp) use: at least `bytes` of it for work queued on s, after a wait for its previous user;
// scrub_scratch_used after the call's last use of it was queued on s (also after a failure).
int scrub_scratch(ppfs_ecc_ctx* c, size_t bytes, hipStream_t s, uint8_t** out);
void scrub_scratch_used(ppfs_ecc_ctx* c, hipStream_t s);

} // namespace ppfs
#pragma GCC visibility pop
