// file_call.hpp -- what the single-file calls (file_path.cpp) and the batch calls (files_path.cpp) share: the walk
// of a call whose arguments are checked and whose plan is built.  Defined in files_path.cpp.
#pragma once

#include <functional>

#include "ctx.hpp"
#pragma GCC visibility push(hidden) // the plan's out-of-line inlines are no part of the library's ABI
#include "files_plan.hpp"

namespace ppfs {

// blocks: resolve the pointers and path statuses; read / write: also the extents and the extent call
enum class FileMode { blocks, read, write };

// One call, device or host form (the pointers are the form's).  The plan has at least one file block; the entry
// point has cleared counts and flags, and the host forms have set `written` to every file's bytes (the device
// walk does that itself, out of the records it uploads).  Whatever a mode does not deliver stays null.
struct FileCall {
    ppfs_ecc_ctx* c;
    uint8_t* image;
    size_t image_blocks;
    // of a Plan or a OnePlan that outlives the call.  plan.one set: a single-file call, whose record goes to the
    // kernels by value and which uploads nothing
    filesplan::PlanView plan;
    FileMode mode;
    int wb;
    uint32_t* index = nullptr;       // blocks: per merged file block
    uint8_t* path_status = nullptr;  // blocks
    uint32_t* tree_index = nullptr;  // blocks: level-major
    uint8_t* tree_status = nullptr;  // blocks
    uint8_t* out = nullptr;          // read: plan.total.bytes bytes
    const uint8_t* in = nullptr;     // write: plan.total.bytes bytes
    uint8_t* status = nullptr;       // read, write: per merged file block
    uint32_t* flags = nullptr;       // a batch: per file
    uint64_t* written = nullptr;     // write: per file
    ppfs_ecc_file_counts* counts = nullptr;
};

// queues the whole walk on the stream, in the context's scrub scratch; queued: call_queued's label
int file_call_device(const FileCall& a, void* stream, const char* queued);
int file_call_host(const FileCall& a);

// Host-built tables into device memory on s, the way of every call that plans on the host (the file batch, the
// directory lookups): fill() writes `bytes` bytes into a page-locked buffer, one copy takes them to d_dst, and the
// buffer returns to the cache once an event recorded behind that copy has completed -- looked at by every later
// staged call, drained at destroy.  The caller's stream is never waited for.  who: the call, for the error text
int stage_upload(ppfs_ecc_ctx* c, uint8_t* d_dst, size_t bytes, hipStream_t s, const char* who, const std::function<void(uint8_t*)>& fill);

} // namespace ppfs
#pragma GCC visibility pop
