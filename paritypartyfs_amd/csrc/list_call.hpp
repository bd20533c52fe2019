// list_call.hpp -- what the block-list calls (list_path.cpp) and the byte-extent calls
// (extent_path.cpp) share: the frame of one device call over the context's row staging, the piece
// size, and which codecs write a corrected block back.  Defined in list_path.cpp.
#pragma once

#include "ctx.hpp"

#pragma GCC visibility push(hidden)
namespace ppfs {

bool has_write_back(const ppfs_ecc_ctx* c); // RS and Hamming: a decode may change the raw block
size_t piece_of(ppfs_ecc_ctx* c);           // blocks per piece of a device list / extent call

// begin(): makes the row staging at the context's first call, orders the call after the last call on
// the stream and after the previous user of the staging (list_ev); end(): records list_ev again, also
// after a failure, and does what every device entry point does after its last launch.
struct ListCall {
    ppfs_ecc_ctx* c;
    hipStream_t s;
    void* stream;
    size_t nblocks;
    int begin();
    int end(int r, const char* what);
};

} // namespace ppfs
#pragma GCC visibility pop
