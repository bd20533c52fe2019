// api.cpp -- host implementation of the ppfs_ecc C ABI (include/ppfs_ecc.h): context create /
// destroy, the device-memory entry points, scrub, vote and groups.  The host-memory entry points
// are in host_path.cpp and the block-list entry points in list_path.cpp; the three share ctx.hpp.
//
// Builds the per-context codec tables (host_tables.hpp: GF(2^8) log/antilog, RS slicing tables, CRC
// shift tables), uploads them once, and dispatches batches to the HIP kernels in rs_kernels.hip and
// bit_kernels.hip (kernels.hpp).  Parameter handling mirrors the reference constructors:
//   ReedSolomonBlockDevice  rs_block_device.cpp:52-60  (n = min(bs,255), t = min(t, n/2))
//   CrcBlockDevice          crc_block_device.cpp:71-76, dataSize :117-120
//   HammingBlockDevice      hamming_block_device.cpp:11-19 (bs = 2^binLog(block_size))
//   ParityBlockDevice       parity_block_device.cpp:9-15
//   RawBlockDevice          raw_block_device.cpp:5-9
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "host_tables.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "resident_plan.hpp"

using namespace ppfs;

thread_local std::string ppfs::g_last_error;

int ppfs::fail(int code, const char* what, hipError_t e)
{
    g_last_error = what;
    if (e != hipSuccess) {
        g_last_error += ": ";
        g_last_error += hipGetErrorString(e);
    }
    return code;
}

// PPFS_ECC_TRACE=1 (diagnostics): timestamped steps of context creation on stderr
void ppfs::trace_step(const char* what)
{
    static const bool on = [] {
        const char* v = std::getenv("PPFS_ECC_TRACE");
        return v && *v && *v != '0';
    }();
    if (!on)
        return;
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    std::fprintf(stderr, "[ppfs_ecc %.6f] %s\n", t, what);
}

// ---------------------------------------------------------------------------------------
// Memory that never synchronizes the device when it is freed.  hipFree and hipHostFree wait for
// every stream of the device, so a context destroyed (or resizing its staging) beside another
// context's resident server, or beside a long kernel of the caller's, waited for them -- 1 to 51 s
// in r3d's destroy test.  Device buffers come from the stream-ordered pool on the context's own
// stream (hipFreeAsync after the work that reads them is known complete); page-locked host
// buffers go back to a process-wide cache (exact size and flags) instead of hipHostFree.
// ---------------------------------------------------------------------------------------
namespace ppfs {
#ifdef PPFS_ECC_DEBUG
// PPFS_ECC_DEBUG: the engine's stream-ordered device allocations, for dma_async's range check
// (the runtime keeps no address-range record for pool memory)
static std::mutex g_pool_mu;
static std::map<uintptr_t, size_t> g_pool;
static void pool_note(void* p, size_t n)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (n)
        g_pool[(uintptr_t)p] = n;
    else
        g_pool.erase((uintptr_t)p);
}
bool pool_covers(const void* p, size_t n)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.upper_bound((uintptr_t)p);
    if (it == g_pool.begin())
        return false;
    --it;
    return (uintptr_t)p >= it->first && (uintptr_t)p + n <= it->first + it->second;
}
#else
static inline void pool_note(void*, size_t) {}
#endif
// hipMallocAsync on stream s (recorded for the debug build's copy checks)
static hipError_t pool_alloc(void** p, size_t n, hipStream_t s)
{
    const hipError_t e = hipMallocAsync(p, n, s);
    if (e == hipSuccess)
        pool_note(*p, n);
    return e;
}
static void pool_free(void* p, hipStream_t s)
{
    if (!p)
        return;
    pool_note(p, 0);
    (void)hipFreeAsync(p, s);
}

hipError_t mem_alloc(ppfs_ecc_ctx* c, void** p, size_t n)
{
    *p = nullptr;
    if (!c->ms) {
        const hipError_t e = hipStreamCreateWithFlags(&c->ms, hipStreamNonBlocking);
        trace_step("mem_alloc: stream created");
        if (e != hipSuccess)
            return e;
    }
    hipError_t e = pool_alloc(p, n, c->ms);
    trace_step("mem_alloc: pool allocation queued");
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->ms); // usable from any stream from here on
    trace_step("mem_alloc: stream synchronized");
    return e;
}
// caller: nothing still queued reads p
void mem_free(ppfs_ecc_ctx* c, void* p)
{
    pool_free(p, c->ms);
}

namespace {
struct PinCache {
    std::mutex mu;
    std::multimap<std::pair<size_t, unsigned>, void*> idle;
    size_t idle_bytes = 0;
    static constexpr size_t kMaxIdle = 512ull << 20;
};
PinCache& pin_cache()
{
    static PinCache* pc = new PinCache(); // never destroyed: buffers may be returned at process exit
    return *pc;
}
} // namespace
hipError_t pin_alloc(void** p, size_t n, unsigned flags)
{
    PinCache& pc = pin_cache();
    {
        std::lock_guard<std::mutex> lk(pc.mu);
        auto it = pc.idle.find({ n, flags });
        if (it != pc.idle.end()) {
            *p = it->second;
            pc.idle.erase(it);
            pc.idle_bytes -= n;
            return hipSuccess;
        }
    }
    return hipHostMalloc(p, n, flags);
}
// caller: nothing still queued reads or writes p
void pin_free(void* p, size_t n, unsigned flags)
{
    if (!p)
        return;
    PinCache& pc = pin_cache();
    {
        std::lock_guard<std::mutex> lk(pc.mu);
        if (pc.idle_bytes + n <= PinCache::kMaxIdle) {
            pc.idle.insert({ { n, flags }, p });
            pc.idle_bytes += n;
            return;
        }
    }
    (void)hipHostFree(p); // beyond the cache: the synchronizing free
}
} // namespace ppfs

namespace {
// Is s capturing a hipGraph?  Work queued then runs later, once per replay, possibly on another
// stream or concurrently with itself.
bool capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return st != hipStreamCaptureStatusNone;
}

// The caller-stream event slot of handle s (-1: none, and with `create` none could be made).
int ev_slot(ppfs_ecc_ctx* c, hipStream_t s, bool create)
{
    int i = 0;
    while (i < c->ev_n && c->ev_stream[i] != s)
        ++i;
    if (i < c->ev_n)
        return i;
    if (!create)
        return -1;
    if (c->ev_n == ppfs_ecc_ctx::kEvSlots
        || hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
        (void)hipGetLastError();
        c->ev_overflow = true;
        return -1;
    }
    c->ev_stream[i] = s;
    c->ev_rec[i] = false;
    c->ev_n++;
    return i;
}

// The context's own host-path streams -- compared only once they exist: before the host path first
// runs they are null, which is also the default stream's handle.
static bool own_stream(const ppfs_ecc_ctx* c, hipStream_t s)
{
    for (hipStream_t h : c->hs)
        if (h && s == h)
            return true;
    return false;
}

// Before a device entry point queues work on caller stream s: order it after the last call queued
// on the same handle.  For the same stream the runtime returns at once (an event recorded on the
// waiting stream itself); it matters when s is a new stream created at the address of a destroyed
// one whose work may still run: the new stream's kernels then never share that work's ticket set
// (ctr_for) or outlive-check (destroy waits on the event re-recorded after this call).
void order_caller_stream(ppfs_ecc_ctx* c, hipStream_t s)
{
    static const bool off = [] { // diagnostics: PPFS_ECC_NO_ORDER=1 skips the wait
        const char* v = std::getenv("PPFS_ECC_NO_ORDER");
        return v && *v && *v != '0';
    }();
    if (off || own_stream(c, s) || capturing(s))
        return;
    const int i = ev_slot(c, s, false);
    if (i >= 0 && c->ev_rec[i] && hipStreamWaitEvent(s, c->ev[i], 0) != hipSuccess)
        (void)hipGetLastError();
}

// The ticket-counter set of stream s (nullptr: the static-walk kernel runs).  A set is shared by
// every launch on its stream, which is safe only because launches on one stream are ordered.  A
// launch captured into a graph gets no set: its replays may run on other streams or overlap each
// other (two kernels on one set would skip or repeat tiles).  A stream without a slot takes a free
// one, or one whose last user's work has completed (its event); with none, or without a caller
// event slot to order it by, it falls back to the static walk.  ppfs_ecc_stream_kernel_name reports
// which path a stream gets.
struct TkSets {
    uint32_t* mine = nullptr;  // the set this launch counts on
    uint32_t* clear = nullptr; // the set it zeroes (the previous launch's)
    int slot = -1, op = 0;
};
// the slot stream s would use (-1: none); with `take`, assign it
int tk_slot(ppfs_ecc_ctx* c, hipStream_t s, bool take)
{
    if (!c->d_ctr || capturing(s))
        return -1;
    const int e = ev_slot(c, s, take);
    if (take && e < 0)
        return -1;
    int i = 0;
    while (i < c->tk_n && c->tk_stream[i] != s)
        ++i;
    if (i == c->tk_n) {
        if (c->tk_n < ppfs_ecc_ctx::kTkSlots) {
            if (take)
                c->tk_n++;
        } else {
            // recycle a slot whose last user's work is complete (the event query is not a wait);
            // the set its next launch counts on was zeroed by that completed work
            i = -1;
            for (int j = 0; j < c->tk_n && i < 0; ++j) {
                if (!c->ev_rec[c->tk_ev[j]]) // its last record failed: nothing tells when it is done
                    continue;
                const hipError_t q = hipEventQuery(c->ev[c->tk_ev[j]]);
                if (q == hipSuccess)
                    i = j;
                else if (q != hipErrorNotReady)
                    (void)hipGetLastError();
            }
            if (i < 0)
                return -1;
        }
        if (take)
            c->tk_stream[i] = s;
    }
    if (take)
        c->tk_ev[i] = e;
    return i;
}
TkSets ctr_for(ppfs_ecc_ctx* c, hipStream_t s, int op /* 0 encode, 1 decode */)
{
    TkSets t;
    const int i = tk_slot(c, s, true);
    if (i < 0)
        return t;
    const int par = c->tk_par[i][op];
    uint32_t* base = c->d_ctr + (size_t)i * 2 * ppfs_ecc_ctx::kTkSetWords + (size_t)op * (ppfs_ecc_ctx::kTkSetWords / 2);
    t.mine = base + (size_t)par * ppfs_ecc_ctx::kTkSetWords;
    t.clear = base + (size_t)(par ^ 1) * ppfs_ecc_ctx::kTkSetWords;
    t.slot = i;
    t.op = op;
    return t;
}
// after a launch with sets t went into the stream: the next launch of its kind uses the other set
// (a launch that failed to enqueue zeroed nothing and counted on nothing: the parity stays)
hipError_t tk_commit(ppfs_ecc_ctx* c, const TkSets& t, hipError_t e)
{
    if (e == hipSuccess && t.slot >= 0)
        c->tk_par[t.slot][t.op] ^= 1;
    return e;
}

// After a device entry point queued work on caller stream s: (re-)record s's completion event.
// Captured work is the graph's: the caller keeps the context alive while graphs that use it exist.
void note_caller_stream(ppfs_ecc_ctx* c, hipStream_t s)
{
    // the context's own streams (destroy drains them) -- compared only once they exist: before the
    // host path first runs they are null, which is also the default stream's handle, and work on
    // the default stream must be tracked like any other caller stream's
    if (own_stream(c, s) || capturing(s))
        return;
    const int i = ev_slot(c, s, true);
    if (i < 0)
        return; // ev_overflow: destroy synchronizes the device
    if (hipEventRecord(c->ev[i], s) != hipSuccess) {
        (void)hipGetLastError();
        c->ev_overflow = true;
        c->ev_rec[i] = false;
        return;
    }
    c->ev_rec[i] = true;
}
} // namespace

extern "C" uint64_t ppfs_ecc_crc_implicit_to_explicit(uint64_t implicit_poly) { return (implicit_poly << 1) + 1; }

extern "C" const char* ppfs_ecc_last_error(void) { return g_last_error.c_str(); }

extern "C" int ppfs_ecc_create(const ppfs_ecc_params* params, int device, ppfs_ecc_ctx** out)
{
    if (!params || !out)
        return fail(PPFS_ECC_EINVAL, "null argument");
    *out = nullptr;
    const ppfs_ecc_params p = *params;
    if (p.block_size == 0 || p.block_size > 4096)
        return fail(PPFS_ECC_EINVAL, "block_size must be in [1, 4096] (MAX_BLOCK_SIZE)");
    ppfs_ecc_ctx* c = new (std::nothrow) ppfs_ecc_ctx();
    if (!c)
        return fail(PPFS_ECC_ENOMEM, "ctx alloc");
    c->p = p;
    c->device = device;
    std::vector<uint8_t> tables;
    switch (p.ecc_type) {
    case PPFS_ECC_NONE:
        c->raw = c->data = p.block_size;
        c->kname = "raw-copy";
        break;
    case PPFS_ECC_REED_SOLOMON: {
        c->rs_n = (int)std::min<uint32_t>(p.block_size, 255);
        const int t = (int)std::min<uint32_t>(p.rs_correctable_bytes, (uint32_t)c->rs_n / 2);
        c->rs_t2 = 2 * t;
        c->raw = (uint32_t)c->rs_n;
        c->data = (uint32_t)(c->rs_n - c->rs_t2);
        c->rs_fast = ppfs_rs_fast_supported(c->rs_n, c->rs_t2) != 0;
        tables.resize(4096 + 8192 + 1024, 0);
        if (c->rs_fast) {
            tables = build_rs_fast_tables(c->rs_t2);
            c->kname = ppfs_rs_fast_path(c->rs_t2);
            // PPFS_ECC_LIST_DIRECT=0: list calls of this context take the staged path (A/B runs)
            const char* ld = std::getenv("PPFS_ECC_LIST_DIRECT");
            c->list_direct = rs_wb_direct(c) && !(ld && ld[0] == '0' && !ld[1]);
            // PPFS_ECC_RESIDENT_MIB: the cache-resident codeword prefix of this context's 2t <= 8 ticket
            // encodes (resident_plan.hpp), 0 = off
            c->resident_bytes = plan::resident_env(std::getenv("PPFS_ECC_RESIDENT_MIB"));
        } else {
            tables.assign(1024 + 256, 0);
            build_gf_block(tables.data());
            std::vector<uint8_t> g = rs_generator(c->rs_t2);
            std::memcpy(tables.data() + 1024, g.data(), g.size());
            c->kname = "rs-generic-lfsr";
        }
        break;
    }
    case PPFS_ECC_CRC: {
        const int n = bitlen64(p.crc_polynomial) - 1;
        if (n < 1 || n > 63) {
            delete c;
            return fail(PPFS_ECC_EINVAL, "CRC polynomial degree must be in [1, 63]");
        }
        const uint32_t nbc = (uint32_t)((n + 7) / 8);
        if (p.block_size <= nbc) {
            delete c;
            return fail(PPFS_ECC_EINVAL, "block too small for the CRC");
        }
        c->crc_n = n;
        c->crc_mask = (1ull << n) - 1;
        c->raw = p.block_size;
        c->data = p.block_size - nbc;
        tables = build_crc_tables(p.crc_polynomial, n, c->data);
        if (ppfs_crc_fast_supported(p.block_size, (uint32_t)n)) {
            const std::vector<uint8_t> f = build_crc_fast_tables(p.crc_polynomial, n, c->data, p.block_size);
            if (f.empty()) {
                delete c;
                return fail(PPFS_ECC_EINVAL, "CRC fast tables: device layout mismatch");
            }
            tables.insert(tables.end(), f.begin(), f.end());
        }
        c->kname = ppfs_crc_fast_supported(p.block_size, (uint32_t)n) ? "crc-piecemap-wave" : "crc-nibble-shift";
        break;
    }
    case PPFS_ECC_HAMMING: {
        int pw = 0;
        while ((1u << (pw + 1)) <= p.block_size)
            pw++;
        c->raw = 1u << pw;
        c->data = c->raw - (uint32_t)((3 * pw + 1 + 7) / 8);
        // raw index of the last payload bit (HammingDataBitsIterator, hamming_block_device.cpp:180-198)
        uint32_t idx = 0;
        for (uint32_t i = 0; i < 8 * c->data; ++i) {
            while ((idx & (idx - 1)) == 0)
                idx++;
            c->ham_L = idx++;
        }
        c->kname = ppfs_bitfast_supported(c->raw) ? "hamming-stream-wave"
                                                  : (c->raw < 8 ? "hamming-tiny" : "hamming-funnel");
        break;
    }
    case PPFS_ECC_PARITY: // block_size 1: no payload, the block's own parity (parity_block_device.cpp:9-15)
        c->raw = p.block_size;
        c->data = p.block_size - 1;
        c->kname = ppfs_bitfast_supported(c->raw) ? "parity-stream-wave" : "parity-popcount";
        break;
    default:
        delete c;
        return fail(PPFS_ECC_EINVAL, "unknown ecc_type");
    }
    DeviceGuard guard(device);
    hipError_t e = guard.err;
    if (e != hipSuccess) {
        delete c;
        return fail(PPFS_ECC_EHIP, "hipSetDevice", e);
    }
    trace_step("create: device set");
    if (c->rs_fast && (c->rs_t2 <= 8 || c->rs_t2 == 32)) { // the ticket kernels (rs_wg_tk.hpp, rs_bs.hpp)
        const size_t cb = sizeof(uint32_t) * ppfs_ecc_ctx::kTkSlots * 2 * ppfs_ecc_ctx::kTkSetWords;
        e = mem_alloc(c, (void**)&c->d_ctr, cb);
        trace_step("create: counters allocated");
        if (e == hipSuccess)
            e = hipMemsetAsync(c->d_ctr, 0, cb, c->ms);
        if (e == hipSuccess)
            e = hipStreamSynchronize(c->ms);
        trace_step("create: counters zeroed");
        if (e != hipSuccess) {
            ppfs_ecc_destroy(c);
            return fail(PPFS_ECC_EHIP, "ticket counters", e);
        }
    }
    if (!tables.empty()) {
        // through a page-locked bounce buffer: the engine never hands pageable memory to a copy
        uint8_t* bounce = nullptr;
        e = mem_alloc(c, (void**)&c->d_tables, tables.size());
        trace_step("create: tables allocated");
        if (e == hipSuccess)
            e = pin_alloc((void**)&bounce, tables.size(), kPinStage);
        trace_step("create: bounce buffer");
        if (e == hipSuccess) {
            std::memcpy(bounce, tables.data(), tables.size());
            e = dma_async(c->d_tables, bounce, tables.size(), hipMemcpyHostToDevice, c->ms);
            if (e == hipSuccess)
                e = hipStreamSynchronize(c->ms);
        }
        trace_step("create: tables uploaded");
        if (bounce) {
            // whatever e is: no copy from the bounce may still be queued when it returns to the cache
            if (e != hipSuccess)
                (void)hipStreamSynchronize(c->ms);
            pin_free(bounce, tables.size(), kPinStage);
        }
        if (e != hipSuccess) {
            ppfs_ecc_destroy(c);
            return fail(PPFS_ECC_EHIP, "table upload", e);
        }
    }
    *out = c;
    return 0;
}

extern "C" void ppfs_ecc_destroy(ppfs_ecc_ctx* c)
{
    if (!c)
        return;
    DeviceGuard guard(c->device);
    // the resident server leaves at `stop` before anything it reads is freed
    const bool srv_gone = !c->srv_stuck && server_halt(c);
    if (c->srv_stream && srv_gone)
        (void)hipStreamDestroy(c->srv_stream);
    // Nothing the context queued may outlive it, and destroy waits for nothing else:
    //  - its own streams (host paths) drain before they are destroyed and before the staging
    //    buffers their copies and kernels use are freed;
    //  - work it queued on caller streams (device entry points: it reads the tables, ticket
    //    counters and scratch freed below) is waited for through the per-stream completion events
    //    note_caller_stream recorded after every call;
    //  - only when more caller streams were used than there are event slots does destroy fall back
    //    to a device-wide synchronize.
    // Other contexts' resident servers and unrelated streams are not waited for.
    for (hipStream_t h : c->hs)
        if (h)
            (void)hipStreamSynchronize(h);
    for (int i = 0; i < c->ev_n; ++i) {
        (void)hipEventSynchronize(c->ev[i]);
        (void)hipEventDestroy(c->ev[i]);
    }
    if (c->ev_overflow && (c->d_tables || c->d_scratch || c->d_ctr || c->d_list || c->d_scrub))
        (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    if (!srv_gone) {
        // a launch that ignored `stop` may still read the tables and the mailbox / zero-copy
        // buffers: leak those rather than free memory under a running kernel
        std::fprintf(stderr, "ppfs_ecc_destroy: resident server did not stop within %d ms; its buffers are leaked\n",
            kSrvStopMs);
        c->d_tables = nullptr;
        c->h_zc = nullptr;
        c->h_box = nullptr;
    }
    // frees that never synchronize the device (mem_free, pin_free)
    for (hipStream_t h : c->hs)
        if (h)
            (void)hipStreamDestroy(h);
    for (int i = 0; i < ppfs_ecc_ctx::kSlots; ++i) {
        for (hipEvent_t e : c->hev[i])
            if (e)
                (void)hipEventDestroy(e);
        pin_free(c->h_pin[i], c->pin_bytes, kPinStage);
        mem_free(c, c->d_stage[i]);
    }
    mem_free(c, c->d_tables);
    mem_free(c, c->d_ctr);
    mem_free(c, c->d_scratch);
    mem_free(c, c->d_list); // list calls ran on caller streams: waited for above
    mem_free(c, c->d_ext);  // ... and so did the extent calls
    mem_free(c, c->d_scrub); // ... and the scrub calls
    for (void* p : c->scrub_old)
        mem_free(c, p);
    for (const ppfs_ecc_ctx::FilesStage& st : c->files_stage) { // the batch calls' table uploads: waited for above
        (void)hipEventSynchronize(st.done);
        (void)hipEventDestroy(st.done);
        pin_free(st.buf, st.bytes, kPinStage);
    }
    if (c->scrub_ev)
        (void)hipEventDestroy(c->scrub_ev);
    if (c->list_ev)
        (void)hipEventDestroy(c->list_ev);
    pin_free(c->h_zc, c->zc_bytes, kPinMapped);
    pin_free(c->h_box, sizeof(ppfs::SrvBox), kPinMapped); // after the streams drained: flag kernels write it
    if (c->ms)
        (void)hipStreamDestroy(c->ms); // its frees complete first
    delete c;
}

extern "C" size_t ppfs_ecc_raw_block_size(const ppfs_ecc_ctx* c) { return c ? c->raw : 0; }
extern "C" size_t ppfs_ecc_data_size(const ppfs_ecc_ctx* c) { return c ? c->data : 0; }
extern "C" const char* ppfs_ecc_kernel_name(const ppfs_ecc_ctx* c) { return c ? c->kname : ""; }
extern "C" const char* ppfs_ecc_list_kernel_name(const ppfs_ecc_ctx* c)
{
    return !c ? "" : c->list_direct ? "rs255-wg-list-lds" : "gather-stage-scatter";
}
extern "C" const char* ppfs_ecc_list_encode_kernel_name(const ppfs_ecc_ctx* c)
{
    return !c ? "" : c->list_direct ? "rs255-wg-list-store-lds" : "gather-stage-scatter";
}

// PPFS_ECC_DEBUG builds: out-of-bounds global accesses the kernels detected and skipped (dbg.hpp),
// summed over the kernel translation units; -1 in normal builds
#ifdef PPFS_ECC_DEBUG
#define PPFS_DBG_UNITS(X) X(ppfs_dbg_faults_rs_t2) X(ppfs_dbg_faults_rs_t4) X(ppfs_dbg_faults_rs_t6) \
    X(ppfs_dbg_faults_rs_t8) X(ppfs_dbg_faults_rs_t10) X(ppfs_dbg_faults_rs_t16) X(ppfs_dbg_faults_rs_t32)   \
    X(ppfs_dbg_faults_rs_generic) X(ppfs_dbg_faults_bit) X(ppfs_dbg_faults_bitfast) X(ppfs_dbg_faults_vote) \
    X(ppfs_dbg_alloc_faults) X(ppfs_dbg_files_faults) X(ppfs_dbg_inode_faults) X(ppfs_dbg_lookup_faults)
#define PPFS_DBG_DECL(f) extern "C" long long f(void);
PPFS_DBG_UNITS(PPFS_DBG_DECL)
extern "C" long long ppfs_ecc_debug_faults(void)
{
    long long sum = 0;
#define PPFS_DBG_ADD(f)                                                                                                \
    {                                                                                                                  \
        const long long v = f();                                                                                       \
        if (v < 0)                                                                                                     \
            return v;                                                                                                  \
        sum += v;                                                                                                      \
    }
    PPFS_DBG_UNITS(PPFS_DBG_ADD)
    return sum;
}
#else
extern "C" long long ppfs_ecc_debug_faults(void) { return -1; }
#endif

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// PPFS_ECC_SYNC_CHECK=1 (debug runs): every device-resident entry point drains its stream and
// reports an asynchronous fault of the work it queued under its own name, instead of at some later
// unrelated call.  Off by default: the entry points are asynchronous.
static bool sync_check_enabled()
{
    static const bool on = [] {
        const char* v = std::getenv("PPFS_ECC_SYNC_CHECK");
        return v && *v && *v != '0';
    }();
    return on;
}

static int sync_check(int r, void* stream, const char* what)
{
    if (r || !sync_check_enabled() || capturing((hipStream_t)stream)) // a capture runs nothing yet
        return r;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess)
        e = hipGetLastError();
    return e != hipSuccess ? fail(PPFS_ECC_EHIP, what, e) : 0;
}

static int ppfs_ecc_encode_device_impl(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_raw, size_t nblocks,
    void* stream)
{
    if (!c || (nblocks && ((!d_data && c->data) || !d_raw)))
        return fail(PPFS_ECC_EINVAL, "encode: null argument");
    if (nblocks == 0)
        return 0;
    hipStream_t s = (hipStream_t)stream;
    switch (c->p.ecc_type) {
    case PPFS_ECC_NONE:
        return check_hip(dma_async(d_raw, d_data, nblocks * c->raw, hipMemcpyDeviceToDevice, s), "copy");
    case PPFS_ECC_REED_SOLOMON:
        if (c->rs_fast && aligned16(d_data) && aligned16(d_raw)) {
            const TkSets t = ctr_for(c, s, 0);
            return check_hip(
                tk_commit(c, t, ppfs_rs_fast_encode(c->rs_t2, d_data, d_raw, nblocks, c->d_tables, s, t.mine, t.clear,
                                plan::resident_tiles(nblocks, c->resident_bytes))),
                "rs encode");
        }
        if (c->rs_fast) {
            // fast tables but unaligned pointers: the generic kernel needs gf block + generator
            return fail(PPFS_ECC_EINVAL, "rs encode: device pointers must be 16-byte aligned");
        }
        return check_hip(ppfs_rs_generic_encode(d_data, d_raw, nblocks, c->rs_n, c->rs_t2, c->d_tables, s),
            "rs generic encode");
    case PPFS_ECC_CRC:
        return check_hip(ppfs_crc_encode(d_data, d_raw, nullptr, nblocks, c->raw, c->data, (uint32_t)c->crc_n,
                             c->crc_mask, c->d_tables, s),
            "crc encode");
    case PPFS_ECC_HAMMING:
        if (c->raw >= 8 && !aligned16(d_raw))
            return fail(PPFS_ECC_EINVAL, "hamming: raw pointer must be 16-byte aligned");
        return check_hip(ppfs_ham_encode(d_data, d_raw, nullptr, nblocks, c->raw, c->data, c->ham_L, s),
            "hamming encode");
    case PPFS_ECC_PARITY:
        return check_hip(ppfs_parity_encode(d_data, d_raw, nullptr, nblocks, c->raw, s), "parity encode");
    }
    return fail(PPFS_ECC_EINVAL, "bad ctx");
}

// wb_dst (the host path only, rs_wb_direct): the write-backs go there instead of into d_raw
static int ppfs_ecc_decode_device_impl(ppfs_ecc_ctx* c, uint8_t* d_raw, uint8_t* d_data, uint8_t* d_status,
    size_t nblocks, int write_back, uint8_t* d_spill, void* stream, uint8_t* wb_dst)
{
    if (!c || (nblocks && !d_raw))
        return fail(PPFS_ECC_EINVAL, "decode: null argument");
    if (nblocks == 0)
        return 0;
    if (wb_dst && !rs_wb_direct(c))
        return fail(PPFS_ECC_EINVAL, "decode: no direct write-back for this codec");
    hipStream_t s = (hipStream_t)stream;
    switch (c->p.ecc_type) {
    case PPFS_ECC_NONE:
        if (d_status) {
            int r = check_hip(hipMemsetAsync(d_status, 0, nblocks, s), "status");
            if (r)
                return r;
        }
        if (d_data)
            return check_hip(dma_async(d_data, d_raw, nblocks * c->raw, hipMemcpyDeviceToDevice, s), "copy");
        return 0;
    case PPFS_ECC_REED_SOLOMON:
        if (c->rs_fast) {
            if (!aligned16(d_raw) || (d_data && !aligned16(d_data)) || (d_status && !aligned16(d_status)))
                return fail(PPFS_ECC_EINVAL, "rs decode: device pointers must be 16-byte aligned");
            if (d_spill) {
                int r = check_hip(hipMemsetAsync(d_spill, 0, nblocks * (256 - (size_t)c->rs_n), s), "spill");
                if (r)
                    return r;
            }
            const TkSets t = ctr_for(c, s, 1);
            return check_hip(tk_commit(c, t,
                                 ppfs_rs_fast_decode(c->rs_t2, d_raw, d_data, d_status, nblocks, c->d_tables, write_back, s,
                                     t.mine, t.clear, wb_dst)),
                "rs decode");
        }
        return check_hip(ppfs_rs_generic_decode(d_raw, d_data, d_status, d_spill, nblocks, c->rs_n, c->rs_t2,
                             write_back, c->d_tables, s),
            "rs generic decode");
    case PPFS_ECC_CRC:
        return check_hip(ppfs_crc_check(d_raw, d_data, d_status, nblocks, c->raw, c->data, (uint32_t)c->crc_n,
                             c->crc_mask, c->d_tables, s),
            "crc check");
    case PPFS_ECC_HAMMING:
        if (c->raw >= 8 && !aligned16(d_raw))
            return fail(PPFS_ECC_EINVAL, "hamming: raw pointer must be 16-byte aligned");
        return check_hip(ppfs_ham_decode(d_raw, d_data, d_status, nblocks, write_back, c->raw, c->data, c->ham_L, s),
            "hamming decode");
    case PPFS_ECC_PARITY:
        return check_hip(ppfs_parity_check(d_raw, d_data, d_status, nblocks, c->raw, s), "parity check");
    }
    return fail(PPFS_ECC_EINVAL, "bad ctx");
}

static int ensure_scratch(ppfs_ecc_ctx* c, size_t bytes, hipStream_t s)
{
    if (c->scratch_bytes >= bytes)
        return 0;
    if (c->d_scratch) {
        // an earlier write on this stream may still read the old scratch status
        HIP_TRY(hipStreamSynchronize(s), "scratch sync");
        mem_free(c, c->d_scratch);
    }
    c->d_scratch = nullptr;
    c->scratch_bytes = 0;
    HIP_TRY(mem_alloc(c, (void**)&c->d_scratch, bytes), "scratch alloc");
    c->scratch_bytes = bytes;
    return 0;
}

static int ppfs_ecc_write_device_impl(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_raw, uint8_t* d_status,
    size_t nblocks, void* stream)
{
    if (!c || (nblocks && ((!d_data && c->data) || !d_raw)))
        return fail(PPFS_ECC_EINVAL, "write: null argument");
    if (nblocks == 0)
        return 0;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* st = d_status;
    if (!st) {
        int r = ensure_scratch(c, (nblocks + 15) & ~(size_t)15, s);
        if (r)
            return r;
        st = c->d_scratch;
    }
    int r = 0;
    switch (c->p.ecc_type) {
    case PPFS_ECC_NONE:
        if (d_status && (r = check_hip(hipMemsetAsync(d_status, 0, nblocks, s), "status")))
            return r;
        return check_hip(dma_async(d_raw, d_data, nblocks * c->raw, hipMemcpyDeviceToDevice, s), "copy");
    case PPFS_ECC_REED_SOLOMON:
        // old block decoded for its status (correction event) only; the new codeword does
        // not depend on it (rs_block_device.cpp:61-93)
        if (c->rs_fast && !aligned16(d_data)) // the encode's rule, before the decode writes a status
            return fail(PPFS_ECC_EINVAL, "rs write: device pointers must be 16-byte aligned");
        if ((r = ppfs_ecc_decode_device(c, d_raw, nullptr, st, nblocks, 0, nullptr, stream)))
            return r;
        return ppfs_ecc_encode_device(c, d_data, d_raw, nblocks, stream);
    case PPFS_ECC_CRC:
        if ((r = check_hip(ppfs_crc_check(d_raw, nullptr, st, nblocks, c->raw, c->data, (uint32_t)c->crc_n,
                               c->crc_mask, c->d_tables, s),
                 "crc check")))
            return r;
        return check_hip(ppfs_crc_encode(d_data, d_raw, st, nblocks, c->raw, c->data, (uint32_t)c->crc_n,
                             c->crc_mask, c->d_tables, s),
            "crc encode");
    case PPFS_ECC_HAMMING:
        if ((r = ppfs_ecc_decode_device(c, d_raw, nullptr, st, nblocks, 1, nullptr, stream)))
            return r;
        return check_hip(ppfs_ham_encode(d_data, d_raw, st, nblocks, c->raw, c->data, c->ham_L, s), "hamming encode");
    case PPFS_ECC_PARITY:
        if ((r = check_hip(ppfs_parity_check(d_raw, nullptr, st, nblocks, c->raw, s), "parity check")))
            return r;
        return check_hip(ppfs_parity_encode(d_data, d_raw, st, nblocks, c->raw, s), "parity encode");
    }
    return fail(PPFS_ECC_EINVAL, "bad ctx");
}

// device entry points: queue, then record the caller stream's completion event (destroy waits
// on it), then (PPFS_ECC_SYNC_CHECK) report an asynchronous fault under the entry's own name
static int queued(ppfs_ecc_ctx* c, int r, size_t nblocks, void* stream, const char* what)
{
    if (!r && nblocks)
        note_caller_stream(c, (hipStream_t)stream);
    return sync_check(r, stream, what);
}
// ... and before it queues anything: after the last call on the same stream handle
static void* ordered(ppfs_ecc_ctx* c, size_t nblocks, void* stream)
{
    if (c && nblocks)
        order_caller_stream(c, (hipStream_t)stream);
    return stream;
}

extern "C" int ppfs_ecc_encode_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_raw, size_t nblocks,
    void* stream)
{
    return queued(c, ppfs_ecc_encode_device_impl(c, d_data, d_raw, nblocks, ordered(c, nblocks, stream)), nblocks,
        stream, "encode (async)");
}

extern "C" int ppfs_ecc_decode_device(ppfs_ecc_ctx* c, uint8_t* d_raw, uint8_t* d_data, uint8_t* d_status,
    size_t nblocks, int write_back, uint8_t* d_spill, void* stream)
{
    return decode_device_to(c, d_raw, d_data, d_status, nblocks, write_back, d_spill, stream, nullptr);
}

int ppfs::decode_device_to(ppfs_ecc_ctx* c, uint8_t* d_raw, uint8_t* d_data, uint8_t* d_status, size_t nblocks,
    int write_back, uint8_t* d_spill, void* stream, uint8_t* wb_dst)
{
    return queued(c,
        ppfs_ecc_decode_device_impl(c, d_raw, d_data, d_status, nblocks, write_back, d_spill, ordered(c, nblocks, stream),
            wb_dst),
        nblocks, stream, "decode (async)");
}

extern "C" int ppfs_ecc_write_device(ppfs_ecc_ctx* c, const uint8_t* d_data, uint8_t* d_raw, uint8_t* d_status,
    size_t nblocks, void* stream)
{
    return queued(c, ppfs_ecc_write_device_impl(c, d_data, d_raw, d_status, nblocks, ordered(c, nblocks, stream)),
        nblocks, stream, "write (async)");
}

bool ppfs::stream_capturing(hipStream_t s) { return capturing(s); }
void* ppfs::call_ordered(ppfs_ecc_ctx* c, size_t nblocks, void* stream) { return ordered(c, nblocks, stream); }
int ppfs::call_queued(ppfs_ecc_ctx* c, int r, size_t nblocks, void* stream, const char* what)
{
    return queued(c, r, nblocks, stream, what);
}

namespace ppfs {
thread_local TimeHook g_time_hook;
}

extern "C" int ppfs_ecc_time_next_launch(void* start_event, void* stop_event)
{
    if ((start_event == nullptr) != (stop_event == nullptr))
        return -EINVAL;
    ppfs::g_time_hook = ppfs::TimeHook { (hipEvent_t)start_event, (hipEvent_t)stop_event };
    return 0;
}

extern "C" const char* ppfs_ecc_stream_kernel_name(ppfs_ecc_ctx* c, void* stream)
{
    if (!c)
        return "";
    if (c->d_ctr && (c->rs_t2 <= 8 || c->rs_t2 == 32)) {
        // 2t <= 8 and 2t = 32: ticket walks while the stream has (or can get) a counter set
        const hipStream_t s = (hipStream_t)stream;
        const bool evok = ev_slot(c, s, false) >= 0 || c->ev_n < ppfs_ecc_ctx::kEvSlots;
        if (!evok || tk_slot(c, s, false) < 0)
            return c->rs_t2 <= 8 ? "rs255-wg-seg4-lds" // rs_wg.hpp static walk
                                 : "rs255-bs-byte-lds-static"; // rs_bs.hpp, BsWalk without counters
    }
    return c->kname;
}

// ---------------------------------------------------------------------------------------
// Whole-image scrub: the effect of readBlock(i) for i = 0..nblocks-1 in order on
// a disk image of image_bytes bytes, without the payloads: RS writes back the corrected
// codeword (rs_block_device.cpp:175-180), Hamming the flipped byte (hamming_block_device.cpp:
// 41-51), CRC and parity only check.  Blocks are independent except in one case: a shortened RS
// code (n < 255) whose miscorrection lands at a position >= n writes those bytes past the block
// end -- into the next block(s), which the sequential reference then reads modified, or off
// the image, in which case HeapDisk::write (heap_disk.cpp:21-27) rejects the whole write-back.
// Scrub reproduces that: one batch pass without write-back finds the spilling blocks (their
// spill record), and the image is then processed in runs between them.
// ---------------------------------------------------------------------------------------
namespace {
struct ScrubOps { // decode a block range of the image; copy spill bytes into the image
    std::function<int(size_t b0, size_t nb, int wb, uint8_t* st, uint8_t* spill)> decode;
    std::function<int(size_t addr, const uint8_t* src, size_t n)> put;
};

int scrub_run(const ppfs_ecc_ctx* c, size_t image_bytes, size_t nblocks, uint8_t* st, const ScrubOps& ops)
{
    const bool wb = has_write_back(c);
    if (!(c->p.ecc_type == PPFS_ECC_REED_SOLOMON && c->rs_n < 255))
        return ops.decode(0, nblocks, wb ? 1 : 0, st, nullptr);
    const size_t n = c->raw, sb = 256 - n;
    std::vector<uint8_t> spill(nblocks * sb);
    int r = ops.decode(0, nblocks, 0, st, spill.data()); // status + spill records, image untouched
    if (r)
        return r;
    size_t start = 0;
    for (size_t i = 0; i < nblocks; ++i) {
        const size_t extra = spill[i * sb];
        if (!extra)
            continue;
        if (i > start && (r = ops.decode(start, i - start, 1, st + start, nullptr)))
            return r;
        const size_t end = (i + 1) * n + extra; // the write-back covers [i n, end)
        if (end <= image_bytes) {
            if ((r = ops.decode(i, 1, 1, st + i, nullptr)) || (r = ops.put((i + 1) * n, &spill[i * sb + 1], extra)))
                return r;
            const size_t j = std::min(nblocks - 1, (end - 1) / n); // last block the spill touched
            if (j > i && (r = ops.decode(i + 1, j - i, 0, st + i + 1, &spill[(i + 1) * sb])))
                return r;
        } // else the reference's disk write fails and nothing of block i is written back
        start = i + 1;
    }
    return start < nblocks ? ops.decode(start, nblocks - start, 1, st + start, nullptr) : 0;
}

void scrub_counts(const uint8_t* st, size_t nblocks, size_t* counts)
{
    if (!counts)
        return;
    counts[0] = counts[1] = counts[2] = 0;
    for (size_t i = 0; i < nblocks; ++i)
        counts[st[i] == PPFS_ECC_OK ? 0 : (st[i] == PPFS_ECC_CORRECTED ? 1 : 2)]++;
}
} // namespace

extern "C" int ppfs_ecc_scrub_host(ppfs_ecc_ctx* c, uint8_t* image, size_t image_bytes, size_t nblocks,
    uint8_t* status, size_t* counts)
{
    if (!c || (nblocks && !image) || image_bytes < nblocks * (size_t)c->raw)
        return fail(PPFS_ECC_EINVAL, "scrub: bad argument");
    std::vector<uint8_t> st_local;
    if (!status) {
        st_local.resize(nblocks);
        status = st_local.data();
    }
    const size_t n = c->raw;
    ScrubOps ops;
    ops.decode = [&](size_t b0, size_t nb, int wb, uint8_t* st, uint8_t* spill) {
        return ppfs_ecc_decode_host(c, image + b0 * n, nullptr, st, nb, wb, spill);
    };
    ops.put = [&](size_t addr, const uint8_t* src, size_t len) {
        std::memcpy(image + addr, src, len);
        return 0;
    };
    const int r = scrub_run(c, image_bytes, nblocks, status, ops);
    if (r)
        return r;
    scrub_counts(status, nblocks, counts);
    return 0;
}

extern "C" int ppfs_ecc_scrub_device(ppfs_ecc_ctx* c, uint8_t* d_image, size_t image_bytes, size_t nblocks,
    uint8_t* d_status, void* stream)
{
    if (!c || (nblocks && !d_image) || image_bytes < nblocks * (size_t)c->raw)
        return fail(PPFS_ECC_EINVAL, "scrub: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = c->raw, sb = spill_bytes(c);
    const bool chain = c->p.ecc_type == PPFS_ECC_REED_SOLOMON && c->rs_n < 255;
    uint8_t* d_spill = nullptr;
    uint8_t* bounce = nullptr; // page-locked: the spill records and patches never DMA pageable memory
    if (chain) {
        HIP_TRY(pool_alloc((void**)&d_spill, nblocks * sb, s), "scrub spill alloc");
        if (pin_alloc((void**)&bounce, std::max<size_t>(nblocks * sb, 256), kPinStage) != hipSuccess) {
            pool_free(d_spill, s);
            return fail(PPFS_ECC_ENOMEM, "scrub spill bounce");
        }
    }
    ScrubOps ops;
    ops.decode = [&](size_t b0, size_t nb, int wb, uint8_t* st_host, uint8_t* spill_host) {
        uint8_t* st = d_status ? d_status + b0 : nullptr;
        (void)st_host;
        int r = ppfs_ecc_decode_device(c, d_image + b0 * n, nullptr, st, nb, wb, spill_host ? d_spill + b0 * sb : nullptr,
            stream);
        if (r || !spill_host)
            return r;
        HIP_TRY(dma_async(bounce, d_spill + b0 * sb, nb * sb, hipMemcpyDeviceToHost, s), "scrub spill D2H");
        HIP_TRY(hipStreamSynchronize(s), "scrub sync");
        std::memcpy(spill_host, bounce, nb * sb);
        return 0;
    };
    ops.put = [&](size_t addr, const uint8_t* src, size_t len) { // len <= 255 - n < 256
        std::memcpy(bounce, src, len);
        HIP_TRY(dma_async(d_image + addr, bounce, len, hipMemcpyHostToDevice, s), "scrub spill H2D");
        HIP_TRY(hipStreamSynchronize(s), "scrub sync"); // the bounce is reused by the next call
        return 0;
    };
    // status bytes live on the device; scrub_run only indexes st (never reads it)
    std::vector<uint8_t> dummy(chain ? nblocks : 0);
    const int r = scrub_run(c, image_bytes, nblocks, dummy.data(), ops);
    if (d_spill) {
        pool_free(d_spill, s);
        (void)hipStreamSynchronize(s); // the bounce's last copy is done before it is freed
    }
    if (bounce)
        pin_free(bounce, std::max<size_t>(nblocks * sb, 256), kPinStage);
    return r;
}

// ---------------------------------------------------------------------------------------
// 2-of-3 bitwise voting of replicated records (vote.hip)
// ---------------------------------------------------------------------------------------
extern "C" int ppfs_vote3_device(const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_c, uint8_t* d_out,
    size_t rec_bytes, size_t nrec, uint32_t* d_damaged, void* stream)
{
    if ((nrec && rec_bytes && (!d_a || !d_b || !d_c || !d_out)))
        return fail(PPFS_ECC_EINVAL, "vote3: null argument");
    if (nrec && !rec_bytes)
        return fail(PPFS_ECC_EINVAL, "vote3: zero record size");
    return sync_check(
        check_hip(ppfs_vote3_launch(d_a, d_b, d_c, d_out, rec_bytes, nrec, d_damaged, (hipStream_t)stream), "vote3"),
        stream, "vote3 (async)");
}

extern "C" int ppfs_copy_device(void* d_dst, const void* d_src, size_t bytes, void* stream)
{
    if (bytes && (!d_dst || !d_src))
        return fail(PPFS_ECC_EINVAL, "copy: null argument");
    return sync_check(
        check_hip(ppfs_copy_launch((uint8_t*)d_dst, (const uint8_t*)d_src, bytes, (hipStream_t)stream), "copy"), stream,
        "copy (async)");
}

extern "C" int ppfs_inject_device(uint8_t* d_raw, size_t stride, size_t nblocks, const uint8_t* d_pos,
    const uint8_t* d_val, int mode, void* stream)
{
    if (nblocks && (!d_raw || !d_pos || !d_val))
        return fail(PPFS_ECC_EINVAL, "inject: null argument");
    if (nblocks && !stride)
        return fail(PPFS_ECC_EINVAL, "inject: zero stride");
    if (mode != 0 && mode != 1)
        return fail(PPFS_ECC_EINVAL, "inject: mode must be 0 (set) or 1 (xor)");
    return sync_check(check_hip(ppfs_inject_launch(d_raw, stride, nblocks, d_pos, d_val, mode, (hipStream_t)stream),
                          "inject"),
        stream, "inject (async)");
}

extern "C" int ppfs_vote3_host(int device, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out,
    size_t rec_bytes, size_t nrec, uint32_t* damaged)
{
    if (nrec && (!rec_bytes || !a || !b || !c || !out))
        return fail(PPFS_ECC_EINVAL, "vote3: bad argument");
    const size_t nbytes = rec_bytes * nrec;
    if (nbytes == 0) {
        if (damaged)
            std::memset(damaged, 0, nrec * sizeof(uint32_t));
        return 0;
    }
    DeviceGuard guard(device);
    HIP_TRY(guard.err, "set device");
    // its own non-blocking stream, drained before anything is freed (not the legacy null stream,
    // which does not order against other non-blocking streams).  The caller's (pageable) buffers
    // are copied by the CPU through page-locked staging, as the engine's host calls do: the DMA
    // engines only ever touch memory this call allocated and still holds.
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "vote3 stream");
    uint8_t *d = nullptr, *h = nullptr;
    const size_t dmg_off = (4 * nbytes + 255) & ~(size_t)255, total = dmg_off + nrec * sizeof(uint32_t);
    // stream-ordered device memory and the page-locked cache: nothing here synchronizes the device
    hipError_t e = pool_alloc((void**)&d, total, s);
    if (e == hipSuccess)
        e = pin_alloc((void**)&h, total, kPinStage);
    if (e == hipSuccess) {
        std::memcpy(h, a, nbytes);
        std::memcpy(h + nbytes, b, nbytes);
        std::memcpy(h + 2 * nbytes, c, nbytes);
        e = dma_async(d, h, 3 * nbytes, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess)
        e = ppfs_vote3_launch(d, d + nbytes, d + 2 * nbytes, d + 3 * nbytes, rec_bytes, nrec,
            damaged ? (uint32_t*)(d + dmg_off) : nullptr, s);
    if (e == hipSuccess)
        e = dma_async(h + 3 * nbytes, d + 3 * nbytes, total - 3 * nbytes, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess)
        e = es;
    if (e == hipSuccess) {
        std::memcpy(out, h + 3 * nbytes, nbytes);
        if (damaged)
            std::memcpy(damaged, h + dmg_off, nrec * sizeof(uint32_t));
    }
    const int r = e != hipSuccess ? fail(PPFS_ECC_EHIP, "vote3", e) : 0;
    if (h)
        pin_free(h, total, kPinStage);
    if (d) {
        pool_free(d, s);
        (void)hipStreamSynchronize(s);
    }
    (void)hipStreamDestroy(s);
    return r;
}

// ---------------------------------------------------------------------------------------
// Page-locking of caller memory (a pinned host mirror of the disk image)
// ---------------------------------------------------------------------------------------
// Registry of the ranges registered through this ABI (start -> bytes): ppfs_ecc_host_registered
// lets a caller (tests/conftest.py) check that no engine-registered range outlives its owner --
// a range still registered after its memory went back to the allocator would let a later,
// unrelated buffer at the same address be treated as page-locked.
namespace {
std::mutex g_reg_mu;
std::map<uintptr_t, size_t> g_reg;
} // namespace

extern "C" int ppfs_ecc_host_register(void* ptr, size_t bytes)
{
    if (!ptr || !bytes)
        return fail(PPFS_ECC_EINVAL, "host_register: bad argument");
    std::lock_guard<std::mutex> lk(g_reg_mu);
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault), "hipHostRegister");
    g_reg[(uintptr_t)ptr] = bytes;
    return 0;
}

extern "C" int ppfs_ecc_host_unregister(void* ptr)
{
    if (!ptr)
        return fail(PPFS_ECC_EINVAL, "host_unregister: null pointer");
    std::lock_guard<std::mutex> lk(g_reg_mu);
    HIP_TRY(hipHostUnregister(ptr), "hipHostUnregister");
    g_reg.erase((uintptr_t)ptr);
    return 0;
}

extern "C" long long ppfs_ecc_host_registered(size_t* bytes)
{
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (bytes) {
        size_t b = 0;
        for (const auto& kv : g_reg)
            b += kv.second;
        *bytes = b;
    }
    return (long long)g_reg.size();
}

// ------------------------------------------------------------------------------------------
// Multi-GPU host path: contiguous shards, one host thread per context
// ------------------------------------------------------------------------------------------
struct ppfs_ecc_group {
    std::vector<ppfs_ecc_ctx*> ctx;
};

extern "C" int ppfs_ecc_group_create(const ppfs_ecc_params* params, const int* devices, int ndevices,
    ppfs_ecc_group** out)
{
    if (!out || !devices || ndevices <= 0)
        return fail(PPFS_ECC_EINVAL, "group: devices");
    *out = nullptr;
    ppfs_ecc_group* g = new (std::nothrow) ppfs_ecc_group();
    if (!g)
        return fail(PPFS_ECC_ENOMEM, "group alloc");
    for (int i = 0; i < ndevices; ++i) {
        ppfs_ecc_ctx* c = nullptr;
        const int r = ppfs_ecc_create(params, devices[i], &c);
        if (r) {
            ppfs_ecc_group_destroy(g);
            return r;
        }
        g->ctx.push_back(c);
    }
    *out = g;
    return 0;
}

extern "C" void ppfs_ecc_group_destroy(ppfs_ecc_group* g)
{
    if (!g)
        return;
    for (ppfs_ecc_ctx* c : g->ctx)
        ppfs_ecc_destroy(c);
    delete g;
}

extern "C" int ppfs_ecc_group_size(const ppfs_ecc_group* g) { return g ? (int)g->ctx.size() : 0; }

extern "C" ppfs_ecc_ctx* ppfs_ecc_group_ctx(ppfs_ecc_group* g, int i)
{
    return (g && i >= 0 && i < (int)g->ctx.size()) ? g->ctx[(size_t)i] : nullptr;
}

namespace {
// run(ctx, first block, count) for every shard on its own thread; the first failing shard's
// code and message come back to the calling thread
int group_run(ppfs_ecc_group* g, size_t nblocks, const std::function<int(ppfs_ecc_ctx*, size_t, size_t)>& run)
{
    if (!g || g->ctx.empty())
        return fail(PPFS_ECC_EINVAL, "null group");
    const size_t G = g->ctx.size();
    if (G == 1 || nblocks < G)
        return run(g->ctx[0], 0, nblocks);
    std::vector<int> rc(G, 0);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    th.reserve(G);
    for (size_t i = 0; i < G; ++i) {
        const size_t b0 = nblocks * i / G, b1 = nblocks * (i + 1) / G;
        th.emplace_back([&, i, b0, b1] {
            rc[i] = run(g->ctx[i], b0, b1 - b0);
            if (rc[i])
                msg[i] = g_last_error;
        });
    }
    for (auto& t : th)
        t.join();
    for (size_t i = 0; i < G; ++i)
        if (rc[i]) {
            g_last_error = msg[i];
            return rc[i];
        }
    return 0;
}
} // namespace

extern "C" int ppfs_ecc_group_encode_host(ppfs_ecc_group* g, const uint8_t* data, uint8_t* raw, size_t nblocks)
{
    return group_run(g, nblocks, [&](ppfs_ecc_ctx* c, size_t b0, size_t nb) {
        return ppfs_ecc_encode_host(c, data + b0 * c->data, raw + b0 * c->raw, nb);
    });
}

extern "C" int ppfs_ecc_group_decode_host(ppfs_ecc_group* g, uint8_t* raw, uint8_t* data, uint8_t* status,
    size_t nblocks, int write_back, uint8_t* spill)
{
    return group_run(g, nblocks, [&](ppfs_ecc_ctx* c, size_t b0, size_t nb) {
        const size_t sp = spill_bytes(c);
        return ppfs_ecc_decode_host(c, raw + b0 * c->raw, data ? data + b0 * c->data : nullptr,
            status ? status + b0 : nullptr, nb, write_back, spill ? spill + b0 * sp : nullptr);
    });
}

extern "C" int ppfs_ecc_group_write_host(ppfs_ecc_group* g, const uint8_t* data, uint8_t* raw, uint8_t* status,
    size_t nblocks)
{
    return group_run(g, nblocks, [&](ppfs_ecc_ctx* c, size_t b0, size_t nb) {
        return ppfs_ecc_write_host(c, data + b0 * c->data, raw + b0 * c->raw, status ? status + b0 : nullptr, nb);
    });
}
