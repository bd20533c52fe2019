// ctx.hpp -- the engine context and what api.cpp (create / destroy, the device entry points, scrub,
// vote, groups), host_path.cpp (the host-memory entry points), list_path.cpp (the block-list entry
// points) and extent_path.cpp (the byte-extent entry points) share.  Everything declared in
// namespace ppfs here has hidden visibility: the library exports the C ABI of include/ppfs_ecc.h
// and the kernel launchers, nothing of this.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ppfs_ecc.h"
#include "host_plan.hpp"
#include "server_box.hpp"

#pragma GCC visibility push(hidden)
namespace ppfs {

// the calling thread's last error message (ppfs_ecc_last_error); fail() sets it and returns code
extern thread_local std::string g_last_error;
int fail(int code, const char* what, hipError_t e = hipSuccess);
inline int check_hip(hipError_t e, const char* what) { return e != hipSuccess ? fail(PPFS_ECC_EHIP, what, e) : 0; }

// Runs a scope on a context's device and restores the caller's current device afterwards
// (the HIP runtime may be shared with the caller's framework, e.g. torch's current device).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        if (prev != dev)
            err = hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

#define HIP_TRY(expr, what)                                                                                            \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess)                                                                                          \
            return ppfs::fail(PPFS_ECC_EHIP, what, _e);                                                                      \
    } while (0)

} // namespace ppfs
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------------------
struct ppfs_ecc_ctx {
    ppfs_ecc_params p {};
    int device = 0;
    // derived
    uint32_t raw = 0, data = 0;
    int rs_n = 0, rs_t2 = 0;
    bool rs_fast = false;
    int crc_n = 0;
    uint64_t crc_mask = 0;
    uint32_t ham_L = 0;
    const char* kname = "";
    // device tables
    uint8_t* d_tables = nullptr;
    // ticket counters of the dynamic-tile t <= 4 encode and decode (rs_wg_tk.hpp): per stream that
    // runs them through this context a slot of two 2,560-byte sets (launch parity), each an encode
    // half then a decode half.  A launch counts on one set and zeroes the other, which the previous
    // launch of the same kind on the stream used (launches on one stream are ordered; no two streams
    // share a slot); tk_par = the set the next launch of each kind uses.  Further streams use the
    // static walk.
    // Ordering (round 4): a slot remembers the caller-stream event slot (ev[] below) of the stream
    // that last launched on it; a slot passes to another stream only once that event has completed,
    // and every device call first waits for the previous call's event on its stream handle, so a
    // stream created at a destroyed stream's address never runs beside a kernel still counting on
    // the old stream's set.
    static constexpr int kTkSlots = 16, kTkSetWords = 1024; // encode 512 words (rs_wq: 32 counters 64 B apart), decode 512
    uint32_t* d_ctr = nullptr;
    hipStream_t tk_stream[kTkSlots] = {};
    uint8_t tk_par[kTkSlots][2] = {};
    int tk_ev[kTkSlots] = {}; // ev[] slot of the slot's last user
    int tk_n = 0;
    // scratch for write_device status when the caller passes none
    uint8_t* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    // host staging (round 5): a stream per link direction, so that chunk i + 1's H2D runs beside
    // chunk i's D2H (with a stream per slot the slots fell into lockstep: both H2Ds, then both
    // D2Hs, one link direction idle at a time); an event per slot orders its kernel after its H2D.
    // hs[0]: H2D copies (SDMA), the small-batch path and decode write-back fix-ups; hs[1]: kernels
    // and D2H copies (the runtime's D2H into page-locked memory is a blit kernel anyway).  Two, not
    // one per stage: a process gets few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and
    // streams beyond them share queues with torch's -- measured: 4 streams ran slower in bench.py's
    // process than in a torch-free one
    static constexpr int kSlots = 3, kHostStreams = 2;
    hipStream_t hs[kHostStreams] = {};
    hipEvent_t hev[kSlots][2] = {}; // per slot: inputs landed, outputs landed
    uint8_t* h_pin[kSlots] = {};
    uint8_t* d_stage[kSlots] = {};
    size_t stage_bytes = 0;
    bool host_eager = false; // the last chunked decode's write-back predictor, where the next one starts
    // zero-copy staging for small host batches (the per-block IBlockDevice calls): coherent
    // host memory the kernels read and write in place, no H2D / D2H
    uint8_t* h_zc = nullptr;
    uint8_t* d_zc = nullptr;
    size_t zc_bytes = 0;
    // resident small-batch server (RS 2t <= 8, server_box.hpp): mailbox, its stream, the current
    // launch generation, the last request number; srv_ok = -1 undecided, 0 off, 1 on
    ppfs::SrvBox* h_box = nullptr;
    ppfs::SrvBox* d_box = nullptr;
    hipStream_t srv_stream = nullptr;
    uint32_t srv_gen = 0, srv_seq = 0, flag_seq = 0;
    bool srv_launched = false;
    int srv_ok = -1;
    // a resident launch that did not leave when asked (server_stop): the context is unusable and
    // destroy leaks what the launch may still read instead of freeing it under it
    bool srv_stuck = false;
    // Completion of the work this context queued on CALLER streams (the device entry points):
    // one fence-free event per stream, re-recorded after every call, so that destroy waits for
    // exactly that work (it reads the tables, counters and scratch destroy frees) and not for the
    // whole device -- other contexts' resident servers, unrelated torch streams.  A stream beyond
    // kEvSlots sets ev_overflow and destroy falls back to a device-wide synchronize.
    static constexpr int kEvSlots = 32;
    hipStream_t ev_stream[kEvSlots] = {};
    hipEvent_t ev[kEvSlots] = {};
    bool ev_rec[kEvSlots] = {}; // recorded at least once
    int ev_n = 0;
    bool ev_overflow = false;
    // the context's own stream for its stream-ordered device allocations (mem_alloc / mem_free)
    hipStream_t ms = nullptr;
    size_t pin_bytes = 0; // bytes of each h_pin[] buffer (pin cache key)
    // block-list calls (list_path.cpp): the gathered rows of one piece and a status array, made at
    // the first list call and shared by every stream of the context -- a list call waits for
    // list_ev, recorded after the previous list call's last kernel, before it touches them
    uint8_t* d_list = nullptr;
    size_t list_bytes = 0, list_status_off = 0;
    hipEvent_t list_ev = nullptr;
    bool list_ev_rec = false;
    // list decodes, encodes and writes go through the one-kernel direct paths (rs_wg_list.hpp): RS(255, 255-2t), 2t <= 8,
    // unless PPFS_ECC_LIST_DIRECT=0 was set when the context was created (list_path.cpp)
    bool list_direct = false;
    // the cache-resident codeword prefix of the 2t <= 8 ticket encode, bytes (resident_plan.hpp): the
    // default, or PPFS_ECC_RESIDENT_MIB as set when the context was created; each encode launch takes
    // plan::resident_tiles(its blocks, this)
    uint64_t resident_bytes = 0;
    // byte-extent calls (extent_path.cpp): the decoded payloads of one piece and the staged index of
    // its entries, made at the first extent call; ordered by list_ev like the rows they go with
    uint8_t* d_ext = nullptr;
    size_t ext_bytes = 0, ext_index_off = 0;
    // list and allocated scrub (scrub_path.cpp): the scratch of one call (bitmap stream, a piece's list and
    // statuses), made at the first call that needs it and replaced by a larger one when a call needs more
    // (the replaced ones are kept until destroy: queued work may still read them); shared by every stream
    // of the context, so a call that uses it waits for scrub_ev, recorded after the previous such call
    uint8_t* d_scrub = nullptr;
    size_t scrub_bytes = 0;
    std::vector<void*> scrub_old;
    hipEvent_t scrub_ev = nullptr;
    bool scrub_ev_rec = false;
    // batch file calls (files_path.cpp): the page-locked buffers whose host-built tables a queued copy may
    // still read, each with the event recorded behind that copy; a buffer returns to the cache once its
    // event has completed (looked at by later batch calls, drained at destroy)
    struct FilesStage {
        void* buf;
        size_t bytes;
        hipEvent_t done;
    };
    std::vector<FilesStage> files_stage;
};

#pragma GCC visibility push(hidden)
namespace ppfs {

// PPFS_ECC_TRACE=1 (diagnostics): timestamped steps of context creation on stderr (api.cpp)
void trace_step(const char* what);

// Memory that never synchronizes the device when it is freed (api.cpp): stream-ordered device
// memory on the context's own stream, page-locked host buffers from a process-wide cache.
hipError_t mem_alloc(ppfs_ecc_ctx* c, void** p, size_t n);
void mem_free(ppfs_ecc_ctx* c, void* p); // caller: nothing still queued reads p
hipError_t pin_alloc(void** p, size_t n, unsigned flags);
void pin_free(void* p, size_t n, unsigned flags); // caller: nothing still queued reads or writes p
constexpr unsigned kPinStage = hipHostMallocDefault, kPinMapped = hipHostMallocMapped | hipHostMallocCoherent;
#ifdef PPFS_ECC_DEBUG
bool pool_covers(const void* p, size_t n); // [p, p + n) inside one of the engine's pool allocations
#endif

// every copy the engine queues (checked in PPFS_ECC_DEBUG builds), and the page-locked test of a
// caller's host range (host_path.cpp)
hipError_t dma_async(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s);
bool host_pinned(const void* p, size_t bytes);

// Ask the resident server launch to leave and wait for it, at most kSrvStopMs; false = it did not
// leave (host_path.cpp)
constexpr int kSrvStopMs = 2000;
bool server_halt(ppfs_ecc_ctx* c);

// The RS(255, 255 - 2t), 2t <= 8 decodes (rs_wg_tk.hpp / rs_wg.hpp) can put their write-backs
// somewhere other than the codewords they read: the host path points them at a page-locked caller
// image mapped into the device, so a chunk's corrections land there with no codeword copy and no
// patch pass (round 6)
inline bool rs_wb_direct(const ppfs_ecc_ctx* c)
{
    return c->p.ecc_type == PPFS_ECC_REED_SOLOMON && c->rs_fast && c->rs_n == 255 && c->rs_t2 <= 8;
}
// ppfs_ecc_decode_device with the write-backs going to wb_dst instead of into d_raw (rs_wb_direct
// contexts only; nullptr: into d_raw) (api.cpp)
int decode_device_to(ppfs_ecc_ctx* c, uint8_t* d_raw, uint8_t* d_data, uint8_t* d_status, size_t nblocks, int write_back,
    uint8_t* d_spill, void* stream, uint8_t* wb_dst);

// RS and Hamming: a decode with write-back may change the raw block
inline bool has_write_back(const ppfs_ecc_ctx* c)
{
    return c->p.ecc_type == PPFS_ECC_REED_SOLOMON || c->p.ecc_type == PPFS_ECC_HAMMING;
}
// bytes of a decode's spill record per block (host_plan.hpp)
inline size_t spill_bytes(const ppfs_ecc_ctx* c) { return plan::spill_bytes(c->raw); }

// What every device entry point does around the work it queues on a caller's stream (api.cpp), for
// the entry points outside api.cpp: call_ordered before the first launch (after the last call on the
// same stream handle), call_queued after the last (the stream's completion event destroy waits on,
// then PPFS_ECC_SYNC_CHECK); stream_capturing: is s capturing a hipGraph?
bool stream_capturing(hipStream_t s);
void* call_ordered(ppfs_ecc_ctx* c, size_t nblocks, void* stream);
int call_queued(ppfs_ecc_ctx* c, int r, size_t nblocks, void* stream, const char* what);

} // namespace ppfs
#pragma GCC visibility pop
