// host_path.cpp -- the host-memory entry points of the ppfs_ecc C ABI (encode / decode / write on
// caller buffers in host memory).  Small batches (the per-block IBlockDevice calls) run in place on
// coherent host memory, through the resident server where the codec has one; everything larger goes
// through the chunk pipeline: triple-buffered page-locked staging, H2D / kernel / D2H overlapped.
// The arithmetic is in host_plan.hpp, the CPU copies in host_copy.hpp; this file holds the HIP side.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "ctx.hpp"
#include "host_plan.hpp"
#include "kernels.hpp"

using namespace ppfs;
using plan::Layout;

// page-locked host memory (hipHostMalloc / hipHostRegister, e.g. ppfs_ecc_host_register): the
// DMA engines can reach it directly, so the host paths skip the CPU copy through staging
static bool host_pinned_byte(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// The whole range [p, p + bytes) must be page-locked before the DMA engines may touch it: a buffer
// that starts inside a registered region and runs past its end would otherwise be DMA'd from / to
// unlocked pages.  The runtime's allocation record of the first byte (hipMemGetAddressRange: the
// hipHostMalloc / hipHostRegister extent) has to cover the last byte; where the runtime keeps no
// such record the range is probed at both ends and every 64 KiB in between.
bool ppfs::host_pinned(const void* p, size_t bytes)
{
    if (!p || !bytes)
        return true;
    const uintptr_t a = (uintptr_t)p, last = a + bytes - 1;
    if (!host_pinned_byte(p) || !host_pinned_byte((const void*)last))
        return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base && size) {
        const uintptr_t b = (uintptr_t)base;
        if (b <= a && last < b + size)
            return true;
    }
    (void)hipGetLastError();
    constexpr uintptr_t kStride = 64 << 10;
    for (uintptr_t q = (a & ~(kStride - 1)) + kStride; q < last; q += kStride)
        if (!host_pinned_byte((const void*)q))
            return false;
    return true;
}

// Device memory over the whole range [p, p + n): both ends device memory and, where the runtime
// keeps an allocation record (hipMalloc; not stream-ordered pool memory), inside one allocation.
[[maybe_unused]] static bool device_range(const void* p, size_t n)
{
    if (!p || !n)
        return true;
#ifdef PPFS_ECC_DEBUG
    if (pool_covers(p, n)) // the engine's own stream-ordered allocations
        return true;
#endif
    auto dev_byte = [](const void* q) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return a.type == hipMemoryTypeDevice;
    };
    const uintptr_t a = (uintptr_t)p, last = a + n - 1;
    if (!dev_byte(p) || !dev_byte((const void*)last))
        return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base && size)
        return (uintptr_t)base <= a && last < (uintptr_t)base + size;
    (void)hipGetLastError();
    return true;
}

[[maybe_unused]] static std::atomic<long long> g_dma_rejects { 0 };

// Every hipMemcpyAsync of the engine.  PPFS_ECC_DEBUG builds check both ends first: a host end
// must be page-locked over its whole range (host_pinned: the engine's own staging, a hipHostMalloc'd
// or ppfs_ecc_host_register'd caller buffer), a device end device memory over its whole range
// (device_range).  A copy that fails the check is refused -- counted (ppfs_ecc_debug_dma_rejects),
// printed, returned as an error -- never handed to the runtime's pageable-copy path or to the DMA
// engines.  Normal builds: the copy as is.
hipError_t ppfs::dma_async(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
#ifdef PPFS_ECC_DEBUG
    if (n) {
        const bool src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
        const bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
        const bool src_ok = src_dev ? device_range(src, n) : host_pinned(src, n);
        const bool dst_ok = dst_dev ? device_range(dst, n) : host_pinned(dst, n);
        if (!src_ok || !dst_ok) {
            const long long k = ++g_dma_rejects;
            if (k <= 16)
                std::fprintf(stderr, "PPFS_ECC_DEBUG: refused copy of %zu B %p -> %p (kind %d): %s end not %s over its range\n",
                    n, src, dst, (int)kind, src_ok ? "destination" : "source",
                    (src_ok ? dst_dev : src_dev) ? "device memory" : "page-locked");
            return hipErrorInvalidValue;
        }
    }
#endif
    return hipMemcpyAsync(dst, src, n, kind, s);
}

extern "C" long long ppfs_ecc_debug_dma_rejects(void)
{
#ifdef PPFS_ECC_DEBUG
    return g_dma_rejects.load();
#else
    return -1;
#endif
}

// Positive control of the copy checks: a copy from malloc'd (pageable) memory and one into a range
// that runs past its device allocation must both be refused.  1 = both refused (the reject counter
// is restored, so the control does not count as a finding), 0 = a check let one through, -1 in
// normal builds.
extern "C" long long ppfs_ecc_debug_dma_selftest(void)
{
#ifdef PPFS_ECC_DEBUG
    const long long before = g_dma_rejects.load();
    uint8_t* pageable = (uint8_t*)std::malloc(4096);
    uint8_t* d = nullptr;
    if (!pageable || hipMalloc(&d, 4096) != hipSuccess) {
        std::free(pageable);
        return 0;
    }
    const bool r1 = dma_async(d, pageable, 4096, hipMemcpyHostToDevice, nullptr) != hipSuccess;
    const bool r2 = dma_async(d + 4096 - 16, d, 32, hipMemcpyDeviceToDevice, nullptr) != hipSuccess;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(nullptr);
    (void)hipFree(d);
    std::free(pageable);
    g_dma_rejects.store(before);
    return (r1 && r2) ? 1 : 0;
#else
    return -1;
#endif
}

// The kSlots staging slots (page-locked + device, `bytes` each), the two host streams and the slots' events
static int ensure_staging(ppfs_ecc_ctx* c, size_t bytes)
{
    if (c->stage_bytes >= bytes)
        return 0;
    for (hipStream_t h : c->hs)
        if (h)
            HIP_TRY(hipStreamSynchronize(h), "staging sync");
    for (int i = 0; i < ppfs_ecc_ctx::kSlots; ++i) {
        pin_free(c->h_pin[i], c->pin_bytes, kPinStage);
        mem_free(c, c->d_stage[i]);
        c->h_pin[i] = nullptr;
        c->d_stage[i] = nullptr;
    }
    c->stage_bytes = c->pin_bytes = 0;
    for (hipStream_t& h : c->hs)
        if (!h)
            HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking), "stream");
    for (int i = 0; i < ppfs_ecc_ctx::kSlots; ++i) {
        for (hipEvent_t& e : c->hev[i])
            if (!e)
                HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
        HIP_TRY(pin_alloc((void**)&c->h_pin[i], bytes, kPinStage), "pinned alloc");
        c->pin_bytes = bytes;
        HIP_TRY(mem_alloc(c, (void**)&c->d_stage[i], bytes), "stage alloc");
    }
    c->stage_bytes = bytes;
    return 0;
}

// Slots per block of a decode's patch list (vote.hip patch_list_kernel) -- RS(255, k): 2 (a block
// with more changed bytes -- up to 2t, one per root of sigma -- comes back whole); Hamming: 1, the
// one corrected byte -- or 0: the codec returns whole codewords (shortened RS, whose write-back
// also spills past the block, and the codecs without a write-back).  PPFS_ECC_PATCH=0: always whole
// codewords (A/B).
static uint32_t patch_slots(const ppfs_ecc_ctx* c)
{
    static const bool off = [] {
        const char* e = std::getenv("PPFS_ECC_PATCH");
        return e && *e == '0';
    }();
    if (off)
        return 0;
    if (c->p.ecc_type == PPFS_ECC_REED_SOLOMON && c->rs_n == 255)
        return 2; // one or two changed bytes (at most 2t; more come back whole)
    if (c->p.ecc_type == PPFS_ECC_HAMMING)
        return 1;
    return 0;
}

// Blocks per chunk of a context's host calls (plan::chunk_blocks; PPFS_ECC_CHUNK_BLOCKS overrides)
static size_t chunk_blocks(const ppfs_ecc_ctx* c)
{
    static const size_t env = plan::chunk_env(std::getenv("PPFS_ECC_CHUNK_BLOCKS"));
    return plan::chunk_blocks(c->raw, env);
}

static Layout layout_for(const ppfs_ecc_ctx* c, size_t nb) { return plan::layout_for(c->data, c->raw, patch_slots(c), nb); }

enum HostOp { OP_ENCODE, OP_DECODE, OP_WRITE };

// one host call: the op and the caller's buffers (null where the op has none or the caller wants none)
struct HostCall {
    HostOp op;
    const uint8_t* data_in;
    uint8_t *data_out, *raw, *status, *spill;
    size_t nblocks;
    int write_back;
};

// Does encode read the old raw block?  (CRC tail bits, Hamming unused bits, parity fix byte)
static bool raw_is_rmw(const ppfs_ecc_ctx* c)
{
    return c->p.ecc_type == PPFS_ECC_HAMMING || c->p.ecc_type == PPFS_ECC_PARITY
        || (c->p.ecc_type == PPFS_ECC_CRC && (c->crc_n % 8) != 0);
}

// The op's kernels over nb blocks of a staging buffer d laid out by L, on stream s -- the small path
// and the chunk pipeline alike.  wb_dst (rs_wb_direct contexts): the decode's write-backs go there
// instead of into d + L.raw.
static int device_op(ppfs_ecc_ctx* c, const HostCall& k, uint8_t* d, const Layout& L, size_t nb, hipStream_t s,
    uint8_t* wb_dst = nullptr)
{
    switch (k.op) {
    case OP_ENCODE:
        return ppfs_ecc_encode_device(c, d + L.data, d + L.raw, nb, s);
    case OP_WRITE:
        return ppfs_ecc_write_device(c, d + L.data, d + L.raw, d + L.status, nb, s);
    case OP_DECODE:
        return decode_device_to(c, d + L.raw, k.data_out ? d + L.data : nullptr, d + L.status, nb, k.write_back,
            k.spill ? d + L.spill : nullptr, s, wb_dst);
    }
    return fail(PPFS_ECC_EINVAL, "bad op");
}

constexpr size_t kSmallBlocks = 64; // one tile: the per-block IBlockDevice calls

// Ask the resident server launch to leave and wait for it, bounded: it polls `stop` every few
// microseconds, so a launch still running after kSrvStopMs has stopped polling (a hung or
// faulted kernel).  Never blocks past the deadline; false = the launch did not leave.
bool ppfs::server_halt(ppfs_ecc_ctx* c)
{
    if (!c->srv_launched)
        return true;
    __atomic_store_n(&c->h_box->stop, 1u, __ATOMIC_RELEASE);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(c->srv_stream);
        if (e != hipErrorNotReady) {
            (void)hipGetLastError();
            c->srv_launched = false;
            return true;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(kSrvStopMs)) {
            c->srv_stuck = true;
            c->srv_ok = 0;
            return false;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// ---- resident small-batch server (server_box.hpp, rs_wg.hpp rs_wg_server_kernel) ----
// every codec (RS: rs_wg / rs255 / rs_pair / generic servers by table layout; CRC, Hamming, parity:
// bit_server_kernel):
// a per-block call posts its request to the resident
// workgroup instead of launching kernels and synchronizing a stream (measured on the box, RS(255,249),
// one block: launch + stream synchronize alone 10.3 us, a whole decode_host call 16.2 us).
// PPFS_ECC_SERVER=0 turns it off (the launch path below).
constexpr uint32_t kSrvIdleUs = 20000; // a launch leaves after 20 ms without a request

static bool server_eligible(ppfs_ecc_ctx* c)
{
    if (c->srv_ok < 0) {
        const char* e = std::getenv("PPFS_ECC_SERVER");
        const bool off = e && e[0] == '0';
        const bool rs = c->p.ecc_type == PPFS_ECC_REED_SOLOMON
            && (!c->rs_fast || c->rs_t2 <= 8 || c->rs_t2 == 10 || c->rs_t2 == 16 || c->rs_t2 == 32);
        // Hamming blocks < 8 bytes run thread-per-block kernels the bit server does not carry
        const bool bit = c->p.ecc_type == PPFS_ECC_CRC || (c->p.ecc_type == PPFS_ECC_HAMMING && c->raw >= 8)
            || c->p.ecc_type == PPFS_ECC_PARITY;
        c->srv_ok = (!off && (rs || bit)) ? 1 : 0;
    }
    return c->srv_ok == 1;
}

// stop the resident launch (if any) and wait until it has returned (bounded, server_halt); an
// error when it did not: the context is then unusable (srv_stuck)
static int server_stop(ppfs_ecc_ctx* c)
{
    if (server_halt(c))
        return 0;
    return fail(PPFS_ECC_EHIP, "small-batch server did not stop: context unusable");
}

static int server_launch(ppfs_ecc_ctx* c)
{
    const uint32_t gen = (++c->srv_gen) & ~ppfs::SRV_EXITED;
    c->srv_gen = gen;
    trace_step("server: launch");
    __atomic_store_n(&c->h_box->stop, 0u, __ATOMIC_RELEASE);
    if (c->p.ecc_type == PPFS_ECC_REED_SOLOMON && c->rs_fast)
        HIP_TRY(ppfs_rs_server_launch(c->rs_t2, c->d_box, c->d_zc, c->zc_bytes, c->d_tables, gen, kSrvIdleUs, c->srv_stream),
            "server launch");
    else if (c->p.ecc_type == PPFS_ECC_REED_SOLOMON)
        HIP_TRY(ppfs_rs_generic_server_launch(c->rs_n, c->rs_t2, c->d_box, c->d_zc, c->zc_bytes, c->d_tables, gen, kSrvIdleUs,
                    c->srv_stream),
            "server launch");
    else
        HIP_TRY(ppfs_bit_server_launch((int)c->p.ecc_type, c->raw, c->data, (uint32_t)c->crc_n, c->crc_mask, c->ham_L, c->d_box,
                    c->d_zc, c->zc_bytes, c->d_tables, gen, kSrvIdleUs, c->srv_stream),
            "server launch");
    c->srv_launched = true;
    return 0;
}

// the context's mailbox (server requests, completion flag of the launch path)
static int ensure_box(ppfs_ecc_ctx* c)
{
    if (c->h_box)
        return 0;
    HIP_TRY(pin_alloc((void**)&c->h_box, sizeof(ppfs::SrvBox), kPinMapped), "mailbox");
    std::memset((void*)c->h_box, 0, sizeof(ppfs::SrvBox));
    HIP_TRY(hipHostGetDevicePointer((void**)&c->d_box, c->h_box, 0), "mailbox map");
    return 0;
}

// Wait for the small-batch launch path's work on stream s: a flag kernel after it stores a fresh
// number into the mailbox and the host spins on it (hipStreamSynchronize's completion signal
// costs ~4 us more per call).  A faulting kernel never lets the flag arrive: the stream is queried
// every few thousand spins and its error returned.
static int wait_flag(ppfs_ecc_ctx* c, hipStream_t s)
{
    int r = ensure_box(c);
    if (r)
        return r;
    const uint32_t v = ++c->flag_seq;
    HIP_TRY(ppfs_flag_launch(&c->d_box->flag, v, s), "flag launch");
    for (uint32_t spin = 1;; ++spin) {
        if (__atomic_load_n(&c->h_box->flag, __ATOMIC_ACQUIRE) == v)
            return 0;
        if ((spin & 4095u) == 0) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady && e != hipSuccess)
                return check_hip(e, "small-batch kernels");
            if (e == hipSuccess && __atomic_load_n(&c->h_box->flag, __ATOMIC_ACQUIRE) != v)
                return fail(PPFS_ECC_EHIP, "small-batch completion flag missing");
        }
    }
}

static int server_call(ppfs_ecc_ctx* c, HostOp op, const Layout& L, size_t nb, int write_back, bool want_data)
{
    using namespace ppfs;
    if (!c->srv_stream) {
        const int r = ensure_box(c);
        if (r)
            return r;
        // The resident launch gets a stream of its own priority level: HIP maps streams of one
        // priority onto GPU_MAX_HW_QUEUES hardware queues, and a stream sharing the server's queue
        // waits behind the resident launch (round 4: another context's creation in a fresh process
        // waited for good; with more hardware queues, or the server at high priority, it did not)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest
            || hipStreamCreateWithPriority(&c->srv_stream, hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(hipStreamCreateWithFlags(&c->srv_stream, hipStreamNonBlocking), "server stream");
        }
    }
    SrvBox* b = c->h_box;
    const SrvLayout sl = srv_layout((uint32_t)nb, c->data, c->raw);
    if (nb < 1 || nb > SRV_MAX_BLOCKS || sl.data != L.data || sl.raw != L.raw || sl.status != L.status)
        return fail(PPFS_ECC_EINVAL, "small-batch server: layout mismatch");
    const SrvCmd sc { (uint32_t)nb, op == OP_ENCODE ? SRV_ENCODE : (op == OP_DECODE ? SRV_DECODE : SRV_WRITE),
        write_back != 0, want_data };
    c->srv_seq = (c->srv_seq + 1) & 0xFFFFu;
    const uint32_t seq = srv_cmd_pack(c->srv_seq, sc);
    __atomic_store_n(&b->cmd, seq, __ATOMIC_RELEASE); // publishes the request and its input bytes
    auto exited = [&]() { return __atomic_load_n(&b->alive, __ATOMIC_ACQUIRE) == (c->srv_gen | SRV_EXITED); };
    if (!c->srv_launched || exited()) {
        const int r = server_launch(c);
        if (r)
            return r;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1;; ++spin) {
        if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq)
            return 0;
        if ((spin & 255u) == 0) {
            if (exited()) { // the launch left (idle / lifetime) without seeing this request
                const int r = server_launch(c);
                if (r)
                    return r;
            } else if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                const bool stopped = server_stop(c) == 0; // bounded: never hangs on a launch that stopped polling
                c->srv_ok = 0; // this context uses the launch path from now on
                if (stopped && __atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq)
                    return 0;
                return fail(PPFS_ECC_EHIP, stopped ? "small-batch server: no answer within 10 s"
                                                   : "small-batch server: no answer within 10 s and did not stop: context unusable");
            }
        }
    }
}

// Small batches run the kernels on coherent host memory in place: no H2D / D2H copies on the
// critical path of a per-block readBlock / writeBlock (each async copy costs microseconds).
static int host_run_small(ppfs_ecc_ctx* c, const HostCall& k)
{
    const size_t nb = k.nblocks;
    const Layout L = layout_for(c, nb);
    if (c->zc_bytes < L.total) {
        if (server_stop(c)) // it holds the buffer's address
            return PPFS_ECC_EHIP;
        if (c->h_zc && c->hs[0])
            HIP_TRY(hipStreamSynchronize(c->hs[0]), "zero-copy sync");
        pin_free(c->h_zc, c->zc_bytes, kPinMapped);
        c->h_zc = c->d_zc = nullptr;
        c->zc_bytes = 0;
        const size_t bytes = std::max(L.total, layout_for(c, kSmallBlocks).total);
        HIP_TRY(pin_alloc((void**)&c->h_zc, bytes, kPinMapped), "zero-copy alloc");
        HIP_TRY(hipHostGetDevicePointer((void**)&c->d_zc, c->h_zc, 0), "zero-copy map");
        c->zc_bytes = bytes;
    }
    if (!c->hs[0])
        HIP_TRY(hipStreamCreateWithFlags(&c->hs[0], hipStreamNonBlocking), "stream");
    uint8_t* h = c->h_zc;
    if (k.op == OP_ENCODE || k.op == OP_WRITE)
        std::memcpy(h + L.data, k.data_in, nb * c->data);
    if (k.op != OP_ENCODE || raw_is_rmw(c))
        std::memcpy(h + L.raw, k.raw, nb * c->raw);
    if (server_eligible(c) && !k.spill) {
        const int r = server_call(c, k.op, L, nb, k.write_back, k.data_out != nullptr);
        if (r)
            return r;
    } else {
        int r = device_op(c, k, c->d_zc, L, nb, c->hs[0]);
        if (!r)
            r = wait_flag(c, c->hs[0]);
        if (r)
            return r;
    }
    if (k.op == OP_ENCODE || k.op == OP_WRITE)
        std::memcpy(k.raw, h + L.raw, nb * c->raw);
    else if (k.write_back) // only the codewords the decode changed (status 1)
        for (size_t b = 0; b < nb; ++b)
            if (h[L.status + b] == 1)
                std::memcpy(k.raw + b * c->raw, h + L.raw + b * c->raw, c->raw);
    if (k.op == OP_DECODE && k.data_out)
        std::memcpy(k.data_out, h + L.data, nb * c->data);
    if (k.status && k.op != OP_ENCODE)
        std::memcpy(k.status, h + L.status, nb);
    if (k.spill)
        std::memcpy(k.spill, h + L.spill, nb * plan::spill_bytes(c->raw));
    return 0;
}

// ---------------------------------------------------------------------------------------
// The chunk pipeline: a call's blocks go through the kSlots staging slots in pieces (plan::ChunkSeq);
// each piece's inputs are queued on the H2D stream, its kernels and D2H copies on the other
// (ctx.hpp: why two streams and three slots), and a slot is drained -- its outputs waited for and
// handed to the caller -- right before it is reused, and at the end of the call.
// ---------------------------------------------------------------------------------------
namespace {

// How a chunk's codewords get back into the caller's image: decided once, when the chunk is queued
enum class RawBack {
    None, // a decode that only checks: they do not
    Queued, // the whole range, its D2H queued behind the kernel: encode and write, a small chunk's single
            // D2H span, and a decode whose predecessor changed many codewords (the predictor, `eager`)
    AfterStatus, // decode: once the status has landed -- nothing for a clean chunk, a packed gather of
                 // the changed rows, or the whole range when more than 1 / kGatherDiv of them changed
    PatchQueued, // decode: the patch list comes back behind the patch kernel (the predictor again) ...
    PatchAfterStatus, // ... or once the status shows a changed block; the host applies it to the image
    PatchKernel, // decode: the patch kernel stores the changed bytes into the mapped caller image
    DecodeKernel, // decode: the decode kernel itself stores its corrections there (rs_wb_direct)
};

bool has_patch_list(RawBack b)
{
    return b == RawBack::PatchQueued || b == RawBack::PatchAfterStatus || b == RawBack::PatchKernel;
}

struct Slot {
    uint8_t *h, *d; // page-locked and device staging, both laid out by the pipeline's Layout
    hipEvent_t in_landed, out_landed;
    size_t b0 = 0, nb = 0; // the chunk in flight: first block, count
    RawBack back = RawBack::None;
    bool busy = false;
};

class ChunkPipeline {
public:
    ChunkPipeline(ppfs_ecc_ctx* c, const HostCall& k, const Layout& L, size_t chunk);
    int run(plan::ChunkSeq seq);

private:
    bool single_d2h(size_t nb) const { return !direct && nb * (n + kd) <= (64u << 10); }
    const uint8_t* status_of(const Slot& s) const { return (direct && k.status) ? k.status + s.b0 : s.h + L.status; }
    RawBack decide(size_t nb) const;
    int queue_inputs(Slot& s);
    int launch(Slot& s);
    int queue_outputs(Slot& s);
    int drain(Slot& s);
    void copy_changed_staged(Slot& s);
    int fetch_after_status(Slot& s);
    int apply_patches(Slot& s);
    int gather_rows_back(Slot& s, const uint32_t* ix, size_t count, uint8_t* image);

    ppfs_ecc_ctx* const c;
    const HostCall k;
    const Layout L;
    const size_t chunk, n, kd, spill_b; // blocks the layout holds; codeword, payload, spill bytes per block
    const hipStream_t s_in, s_out;
    // every caller buffer page-locked: DMA straight between it and the device staging buffers
    const bool direct;
    // decode with write-back: the codewords come back only where the decode changed them
    // (status 1), read from the chunk's status once it has landed
    const bool lazy_raw;
    // ... and as a patch list (the changed bytes) where the codec bounds them (patch_slots): the
    // host writes those bytes into its image instead of taking back whole codewords
    const uint32_t S;
    // a page-locked caller image the device can address: the patch kernel stores the changed bytes
    // straight into it (no list, no host work); else the list comes back and the host applies it
    uint8_t* img_dev = nullptr;
    // RS with 2t <= 8 into such an image: the decode kernel itself stores its corrections there
    // (rs_wb_direct), so no codeword copy before it and no patch kernel after it
    bool wb_direct = false;
    // predictor: the last drained chunk changed many codewords -> fetch the next ones eagerly
    // (queued behind the kernel, as encode does) instead of after the status has landed.  It starts
    // where the context's previous call left it: the first kSlots chunks are queued before any has
    // landed
    bool eager;
    Slot slots[ppfs_ecc_ctx::kSlots];
};

ChunkPipeline::ChunkPipeline(ppfs_ecc_ctx* c_, const HostCall& k_, const Layout& L_, size_t chunk_)
    : c(c_), k(k_), L(L_), chunk(chunk_), n(c_->raw), kd(c_->data), spill_b(plan::spill_bytes(c_->raw)), s_in(c_->hs[0]),
      s_out(c_->hs[1]),
      direct(host_pinned(k.data_in, k.nblocks * kd) && host_pinned(k.data_out, k.nblocks * kd)
          && host_pinned(k.raw, k.nblocks * n) && host_pinned(k.status, k.nblocks)
          && host_pinned(k.spill, k.nblocks * spill_b)),
      lazy_raw(k.op == OP_DECODE && k.write_back), S(lazy_raw ? patch_slots(c_) : 0u), eager(c_->host_eager)
{
    if (S && direct && hipHostGetDevicePointer((void**)&img_dev, k.raw, 0) != hipSuccess) {
        (void)hipGetLastError();
        img_dev = nullptr;
    }
    wb_direct = img_dev && rs_wb_direct(c);
    for (int i = 0; i < ppfs_ecc_ctx::kSlots; ++i)
        slots[i] = Slot { c->h_pin[i], c->d_stage[i], c->hev[i][0], c->hev[i][1] };
}

RawBack ChunkPipeline::decide(size_t nb) const
{
    if (k.op != OP_DECODE)
        return RawBack::Queued;
    if (!lazy_raw)
        return RawBack::None;
    if (wb_direct)
        return RawBack::DecodeKernel;
    // patch lists for the big chunks (the small-batch path takes its whole staging span back)
    if (S && !single_d2h(nb))
        return img_dev ? RawBack::PatchKernel : (eager ? RawBack::PatchQueued : RawBack::PatchAfterStatus);
    return (single_d2h(nb) || eager) ? RawBack::Queued : RawBack::AfterStatus;
}

int ChunkPipeline::queue_inputs(Slot& s)
{
    // inputs host -> pinned -> device (data and raw regions are adjacent in the layout)
    const size_t b0 = s.b0, nb = s.nb;
    const bool need_data = k.op == OP_ENCODE || k.op == OP_WRITE;
    const bool need_raw = k.op != OP_ENCODE || raw_is_rmw(c);
    if (direct) {
        if (need_data)
            HIP_TRY(dma_async(s.d + L.data, k.data_in + b0 * kd, nb * kd, hipMemcpyHostToDevice, s_in), "H2D data");
        if (need_raw)
            HIP_TRY(dma_async(s.d + L.raw, k.raw + b0 * n, nb * n, hipMemcpyHostToDevice, s_in), "H2D raw");
    } else {
        CopySeg seg[2];
        int ns = 0;
        if (need_data)
            seg[ns++] = { s.h + L.data, k.data_in + b0 * kd, nb * kd };
        if (need_raw)
            seg[ns++] = { s.h + L.raw, k.raw + b0 * n, nb * n };
        par_memcpy_n(seg, ns);
        const size_t in_lo = need_data ? L.data : L.raw;
        const size_t in_hi = need_raw ? L.raw + nb * n : L.data + nb * kd;
        HIP_TRY(dma_async(s.d + in_lo, s.h + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, s_in), "H2D");
    }
    if (has_patch_list(s.back)) // the codewords as they came, for the patch list after the decode (on the input
        // stream, which a decode leaves half idle, not ahead of the kernel on the output stream)
        HIP_TRY(ppfs_copy_launch(s.d + L.orig, s.d + L.raw, nb * n, s_in), "orig copy");
    HIP_TRY(hipEventRecord(s.in_landed, s_in), "event");
    HIP_TRY(hipStreamWaitEvent(s_out, s.in_landed, 0), "wait");
    return 0;
}

int ChunkPipeline::launch(Slot& s)
{
    return device_op(c, k, s.d, L, s.nb, s_out, s.back == RawBack::DecodeKernel ? img_dev + s.b0 * n : nullptr);
}

// outputs device -> pinned staging (or straight to page-locked caller buffers)
int ChunkPipeline::queue_outputs(Slot& s)
{
    const size_t b0 = s.b0, nb = s.nb;
    const bool want_data = k.op == OP_DECODE && k.data_out;
    const bool want_st = (k.status || lazy_raw) && k.op != OP_ENCODE;
    if (single_d2h(nb)) {
        // small batches (the per-block IBlockDevice calls): one D2H of the staging span
        // instead of up to four -- each copy is a few us of latency on the critical path
        const size_t lo = want_data ? L.data : L.raw;
        const size_t hi = k.spill ? L.spill + nb * spill_b : (want_st ? L.status + nb : L.raw + nb * n);
        HIP_TRY(dma_async(s.h + lo, s.d + lo, hi - lo, hipMemcpyDeviceToHost, s_out), "D2H");
    } else {
        uint8_t* o_raw = direct ? k.raw + b0 * n : s.h + L.raw;
        uint8_t* o_data = direct ? (k.data_out ? k.data_out + b0 * kd : nullptr) : s.h + L.data;
        uint8_t* o_st = (direct && k.status) ? k.status + b0 : s.h + L.status;
        uint8_t* o_sp = direct ? (k.spill ? k.spill + b0 * spill_b : nullptr) : s.h + L.spill;
        if (s.back == RawBack::Queued)
            HIP_TRY(dma_async(o_raw, s.d + L.raw, nb * n, hipMemcpyDeviceToHost, s_out), "D2H raw");
        if (want_data)
            HIP_TRY(dma_async(o_data, s.d + L.data, nb * kd, hipMemcpyDeviceToHost, s_out), "D2H data");
        if (want_st)
            HIP_TRY(dma_async(o_st, s.d + L.status, nb, hipMemcpyDeviceToHost, s_out), "D2H status");
        if (k.spill)
            HIP_TRY(dma_async(o_sp, s.d + L.spill, nb * spill_b, hipMemcpyDeviceToHost, s_out), "D2H spill");
        if (has_patch_list(s.back)) {
            HIP_TRY(ppfs_patch_list_launch(s.d + L.raw, s.d + L.orig, s.d + L.status, (uint32_t)n, nb, S,
                        (uint32_t*)(s.d + L.patch), s.back == RawBack::PatchKernel ? img_dev + b0 * n : nullptr, s_out),
                "patch list");
            if (s.back == RawBack::PatchQueued)
                HIP_TRY(dma_async(s.h + L.patch, s.d + L.patch, nb * S * sizeof(uint32_t), hipMemcpyDeviceToHost, s_out),
                    "D2H patch");
        }
    }
    HIP_TRY(hipEventRecord(s.out_landed, s_out), "event");
    return 0;
}

// rows ix[0 .. count) of the slot's codewords, packed by one gather kernel, into image (the
// chunk's first codeword).  The chunk has landed: its staging is idle until reused.  On the H2D
// stream, whose queue holds at most the next kSlots - 1 chunks' input copies; the other holds
// their kernels.  ix lies in the slot's page-locked idx region.
int ChunkPipeline::gather_rows_back(Slot& s, const uint32_t* ix, size_t count, uint8_t* image)
{
    HIP_TRY(dma_async(s.d + L.idx, ix, count * sizeof(uint32_t), hipMemcpyHostToDevice, s_in), "H2D idx");
    HIP_TRY(ppfs_gather_rows_launch(s.d + L.raw, s.nb, s.d + L.gat, (const uint32_t*)(s.d + L.idx), (uint32_t)count,
                (uint32_t)n, s_in),
        "gather");
    HIP_TRY(dma_async(s.h + L.gat, s.d + L.gat, count * n, hipMemcpyDeviceToHost, s_in), "D2H gather");
    HIP_TRY(hipStreamSynchronize(s_in), "sync");
    for (size_t j = 0; j < count; ++j)
        std::memcpy(image + (size_t)ix[j] * n, s.h + L.gat + j * n, n);
    return 0;
}

// RawBack::Queued of a decode: the whole range came back.  Into a page-locked image directly (the
// unchanged blocks got the same bytes again); from staging, the host copies what changed.
void ChunkPipeline::copy_changed_staged(Slot& s)
{
    const uint8_t* sts = status_of(s);
    const plan::Changed chg = plan::scan_changed(sts, s.nb, nullptr);
    eager = chg.eager;
    if (direct || chg.count == 0)
        return;
    uint8_t* img = k.raw + s.b0 * n;
    if (eager)
        par_memcpy(img, s.h + L.raw, s.nb * n);
    else
        for (size_t b = 0; b < s.nb; ++b)
            if (sts[b] == 1)
                std::memcpy(img + b * n, s.h + L.raw + b * n, n);
}

int ChunkPipeline::fetch_after_status(Slot& s)
{
    uint32_t* ix = (uint32_t*)(s.h + L.idx);
    const plan::Changed chg = plan::scan_changed(status_of(s), s.nb, ix);
    eager = chg.eager;
    if (chg.count == 0)
        return 0;
    uint8_t* img = k.raw + s.b0 * n;
    if (!chg.eager)
        return gather_rows_back(s, ix, chg.count, img);
    // many: the whole range (on the H2D stream, like the gather)
    HIP_TRY(dma_async(direct ? img : s.h + L.raw, s.d + L.raw, s.nb * n, hipMemcpyDeviceToHost, s_in), "D2H raw");
    HIP_TRY(hipStreamSynchronize(s_in), "sync");
    if (!direct)
        par_memcpy(img, s.h + L.raw, s.nb * n);
    return 0;
}

// The chunk's patch list into the caller's image: taken back now unless it came behind the
// kernel (the predictor expected many changed blocks), nothing for a clean chunk; blocks with
// more changed bytes than their S slots come back whole, by gathers of at most the gat region's rows.
int ChunkPipeline::apply_patches(Slot& s)
{
    const uint8_t* sts = status_of(s);
    const plan::Changed chg = plan::scan_changed(sts, s.nb, nullptr);
    eager = chg.eager;
    if (chg.count == 0)
        return 0;
    if (s.back == RawBack::PatchAfterStatus) {
        HIP_TRY(dma_async(s.h + L.patch, s.d + L.patch, s.nb * S * sizeof(uint32_t), hipMemcpyDeviceToHost, s_in),
            "D2H patch");
        HIP_TRY(hipStreamSynchronize(s_in), "sync");
    }
    uint8_t* img = k.raw + s.b0 * n;
    const std::vector<uint32_t> over = plan::apply_patch_list(img, n, sts, (const uint32_t*)(s.h + L.patch), S, s.nb,
        plan::patch_pooled(s.nb, chg.count));
    uint32_t* ix = (uint32_t*)(s.h + L.idx);
    for (size_t i = 0; i < over.size(); i += plan::gather_rows(s.nb)) {
        const size_t m = std::min(plan::gather_rows(s.nb), over.size() - i);
        std::copy(over.begin() + i, over.begin() + i + m, ix);
        if (const int r = gather_rows_back(s, ix, m, img))
            return r;
    }
    return 0;
}

// Wait for the slot's chunk and hand its outputs to the caller.  A slot is reused only after this
// saw its outputs land: its H2D then never overwrites staging an earlier chunk's kernel or D2H
// still reads.
int ChunkPipeline::drain(Slot& s)
{
    if (!s.busy)
        return 0;
    HIP_TRY(hipEventSynchronize(s.out_landed), "sync");
    int r = 0;
    switch (s.back) {
    case RawBack::None:
    case RawBack::PatchKernel: // the write-back went straight into the caller's image
    case RawBack::DecodeKernel:
        break;
    case RawBack::Queued:
        if (lazy_raw)
            copy_changed_staged(s);
        break;
    case RawBack::AfterStatus:
        r = fetch_after_status(s);
        break;
    case RawBack::PatchQueued:
    case RawBack::PatchAfterStatus:
        r = apply_patches(s);
        break;
    }
    if (r)
        return r;
    if (!direct) {
        const size_t b0 = s.b0, nb = s.nb;
        CopySeg seg[2];
        int ns = 0;
        if (k.op == OP_ENCODE || k.op == OP_WRITE)
            seg[ns++] = { k.raw + b0 * n, s.h + L.raw, nb * n };
        if (k.op == OP_DECODE && k.data_out)
            seg[ns++] = { k.data_out + b0 * kd, s.h + L.data, nb * kd };
        par_memcpy_n(seg, ns);
        if (k.status)
            std::memcpy(k.status + b0, s.h + L.status, nb);
        if (k.spill)
            std::memcpy(k.spill + b0 * spill_b, s.h + L.spill, nb * spill_b);
    }
    s.busy = false;
    return 0;
}

int ChunkPipeline::run(plan::ChunkSeq seq)
{
    constexpr int NS = ppfs_ecc_ctx::kSlots;
    int i = 0, r = 0;
    for (size_t b0 = 0, nb; (nb = seq.next()) != 0; b0 += nb, i = (i + 1) % NS) {
        if (nb > chunk)
            return fail(PPFS_ECC_EINVAL, "host path: a piece larger than the staging layout");
        Slot& s = slots[i];
        if ((r = drain(s)))
            return r;
        s.b0 = b0;
        s.nb = nb;
        s.back = decide(nb);
        if ((r = queue_inputs(s)) || (r = launch(s)) || (r = queue_outputs(s)))
            return r;
        s.busy = true;
    }
    for (int j = 0; j < NS; ++j) // oldest first
        if ((r = drain(slots[(i + j) % NS])))
            return r;
    if (lazy_raw)
        c->host_eager = eager;
    return 0;
}

} // namespace

static int host_run_chunks(ppfs_ecc_ctx* c, const HostCall& k)
{
    const plan::ChunkSeq seq(k.nblocks, chunk_blocks(c));
    const Layout L = layout_for(c, seq.chunk);
    if (const int r = ensure_staging(c, L.total))
        return r;
    return ChunkPipeline(c, k, L, seq.chunk).run(seq);
}

// A host call returns only once nothing it queued is still in flight: on an error part-way through
// (a failed copy or launch in one slot) the other slots' H2D / kernel / D2H may still be running,
// and their DMA targets the caller's buffers (direct mode) and the staging the next call reuses.
// Every stream is drained before the error goes back; the first error's message is kept.
static int host_run(ppfs_ecc_ctx* c, const HostCall& k)
{
    if (!c)
        return fail(PPFS_ECC_EINVAL, "null ctx");
    if (c->srv_stuck)
        return fail(PPFS_ECC_EHIP, "context unusable: its resident server launch did not stop");
    if (k.nblocks == 0)
        return 0;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err, "set device");
    const int r = k.nblocks <= kSmallBlocks ? host_run_small(c, k) : host_run_chunks(c, k);
    if (r) {
        const std::string msg = g_last_error;
        for (hipStream_t h : c->hs)
            if (h)
                (void)hipStreamSynchronize(h);
        g_last_error = msg;
    }
    return r;
}

extern "C" size_t ppfs_ecc_host_chunk_blocks(ppfs_ecc_ctx* c) { return c ? chunk_blocks(c) : 0; }

extern "C" int ppfs_ecc_encode_host(ppfs_ecc_ctx* c, const uint8_t* data, uint8_t* raw, size_t nblocks)
{
    return host_run(c, HostCall { OP_ENCODE, data, nullptr, raw, nullptr, nullptr, nblocks, 0 });
}

extern "C" int ppfs_ecc_decode_host(ppfs_ecc_ctx* c, uint8_t* raw, uint8_t* data, uint8_t* status, size_t nblocks,
    int write_back, uint8_t* spill)
{
    return host_run(c, HostCall { OP_DECODE, nullptr, data, raw, status, spill, nblocks, write_back });
}

extern "C" int ppfs_ecc_write_host(ppfs_ecc_ctx* c, const uint8_t* data, uint8_t* raw, uint8_t* status, size_t nblocks)
{
    return host_run(c, HostCall { OP_WRITE, data, nullptr, raw, status, nullptr, nblocks, 0 });
}
