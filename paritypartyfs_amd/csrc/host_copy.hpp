// host_copy.hpp -- the CPU side of the pageable host path: threaded, non-temporal copies between a
// caller's buffers and the page-locked staging, and the worker pool they (and the patch-list
// application, host_plan.hpp) run on.  Plain C++, no HIP: tests/cpp/test_host_plan.cpp builds it
// with the host compiler alone.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <pthread.h>
#include <thread>
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#define PPFS_HOST_X86 1
#else
#define PPFS_HOST_X86 0
#endif

namespace {

// Host staging copies of the pageable host path (caller buffer <-> page-locked staging): one CPU
// thread moves ~10 GB/s, well under the link rate the page-locked path reaches, so copies of
// >= 2 MiB are split in 512 KiB pieces over PPFS_ECC_COPY_THREADS threads (default 8 -- the
// calling thread and 7 pool workers; 1 = single-threaded).  The workers persist (a spawn per copy
// cost ~10-20 us a thread), and one job carries every region of a chunk (payload and codewords).
inline int copy_threads()
{
    static const int n = [] {
        const char* e = std::getenv("PPFS_ECC_COPY_THREADS");
        const int v = e ? std::atoi(e) : 8;
        return v < 1 ? 1 : (v > 16 ? 16 : v);
    }();
    return n;
}

// Streaming copy of one staging piece (round 5, PPFS_ECC_COPY_NT=0: plain memcpy): 64-byte
// non-temporal stores skip the read-for-ownership of every destination line, so the copy moves
// its bytes once instead of twice -- the destinations (the page-locked staging the DMA reads, or
// a multi-MB caller buffer) do not fit in the caches anyway.  AVX-512 or AVX2 by the CPU, memcpy
// for the unaligned head and the tail; an sfence makes the stores visible before the job's
// completion is published.  x86 hosts only; elsewhere piece_copy is a memcpy.
#if PPFS_HOST_X86
inline __attribute__((target("avx512f"))) void nt_copy512(uint8_t* d, const uint8_t* s, size_t n)
{
    size_t i = 0;
    for (; i + 256 <= n; i += 256) {
        const __m512i a = _mm512_loadu_si512((const void*)(s + i)), b = _mm512_loadu_si512((const void*)(s + i + 64));
        const __m512i c = _mm512_loadu_si512((const void*)(s + i + 128)), e = _mm512_loadu_si512((const void*)(s + i + 192));
        _mm512_stream_si512((__m512i*)(d + i), a);
        _mm512_stream_si512((__m512i*)(d + i + 64), b);
        _mm512_stream_si512((__m512i*)(d + i + 128), c);
        _mm512_stream_si512((__m512i*)(d + i + 192), e);
    }
    for (; i + 64 <= n; i += 64)
        _mm512_stream_si512((__m512i*)(d + i), _mm512_loadu_si512((const void*)(s + i)));
    if (i < n)
        std::memcpy(d + i, s + i, n - i);
}
inline __attribute__((target("avx2"))) void nt_copy256(uint8_t* d, const uint8_t* s, size_t n)
{
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256((const __m256i*)(s + i)), b = _mm256_loadu_si256((const __m256i*)(s + i + 32));
        const __m256i c = _mm256_loadu_si256((const __m256i*)(s + i + 64)), e = _mm256_loadu_si256((const __m256i*)(s + i + 96));
        _mm256_stream_si256((__m256i*)(d + i), a);
        _mm256_stream_si256((__m256i*)(d + i + 32), b);
        _mm256_stream_si256((__m256i*)(d + i + 64), c);
        _mm256_stream_si256((__m256i*)(d + i + 96), e);
    }
    if (i < n)
        std::memcpy(d + i, s + i, n - i);
}
#endif
inline void piece_copy(void* dst, const void* src, size_t n)
{
#if !PPFS_HOST_X86
    std::memcpy(dst, src, n);
#else
    static const int mode = [] { // 2 AVX-512, 1 AVX2, 0 memcpy
        const char* e = std::getenv("PPFS_ECC_COPY_NT");
        if (e && *e == '0')
            return 0;
        // the CPU's flags from /proc/cpuinfo (this TU is also parsed for the GPU, where the
        // compiler's CPU-feature builtins do not exist)
        bool a512 = false, a2 = false;
        if (FILE* f = std::fopen("/proc/cpuinfo", "r")) {
            char line[8192];
            while (std::fgets(line, sizeof(line), f))
                if (std::strncmp(line, "flags", 5) == 0) {
                    a512 = std::strstr(line, " avx512f") != nullptr;
                    a2 = std::strstr(line, " avx2") != nullptr;
                    break;
                }
            std::fclose(f);
        }
        return a512 ? 2 : (a2 ? 1 : 0);
    }();
    uint8_t* d = (uint8_t*)dst;
    const uint8_t* s = (const uint8_t*)src;
    if (mode == 0 || n < 4096) {
        std::memcpy(d, s, n);
        return;
    }
    const size_t head = (64 - ((uintptr_t)d & 63)) & 63; // stores 64-byte aligned
    std::memcpy(d, s, head);
    if (mode == 2)
        nt_copy512(d + head, s + head, n - head);
    else
        nt_copy256(d + head, s + head, n - head);
    _mm_sfence();
#endif
}

struct CopySeg {
    void* dst;
    const void* src;
    size_t n;
};

class CopyPool {
    struct Job;

public:
    static constexpr size_t kPiece = 512u << 10;
    static constexpr int kMaxSegs = 4;

    // one pool per process, its workers blocked on cv_ between jobs; leaked at exit (the workers
    // never touch freed state).  Never used in a forked child (par_memcpy_n): the parent's workers
    // do not exist there, and a mutex another parent thread held at the fork stays locked.
    static CopyPool& get()
    {
        static CopyPool* pool = new CopyPool(copy_threads() - 1);
        return *pool;
    }

    void run(const CopySeg* segs, int nseg)
    {
        Job j;
        for (int i = 0; i < nseg; ++i) {
            j.seg[i] = segs[i];
            j.first[i + 1] = j.first[i] + (segs[i].n + kPiece - 1) / kPiece;
        }
        j.nseg = nseg;
        j.total = j.first[nseg];
        submit(j);
    }

    // fn(i) for i in [0, n), spread over the workers and the caller
    void run_for(size_t n, const std::function<void(size_t)>& fn)
    {
        Job j;
        j.fn = &fn;
        j.total = n;
        submit(j);
    }

private:
    void submit(Job& j)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &j;
            ++gen_;
        }
        cv_.notify_all();
        work(j);
        std::unique_lock<std::mutex> lk(m_);
        if (job_ == &j) // late wakers find no job (concurrent callers: each one finishes its own job)
            job_ = nullptr;
        done_.wait(lk, [&] { return j.finished.load() == j.total && j.users == 0; });
    }

    struct Job {
        CopySeg seg[kMaxSegs] {};
        size_t first[kMaxSegs + 1] {}; // first piece of each segment
        int nseg = 0;
        size_t total = 0;
        std::atomic<size_t> next { 0 }, finished { 0 };
        int users = 0; // workers holding the job (guarded by m_)
        const std::function<void(size_t)>* fn = nullptr; // run_for: item p is fn(p), not a copy piece
    };

    explicit CopyPool(int workers)
    {
        for (int i = 0; i < workers; ++i)
            std::thread([this] { loop(); }).detach();
    }

    void work(Job& j)
    {
        size_t done = 0;
        for (size_t p; (p = j.next.fetch_add(1)) < j.total; ++done) {
            if (j.fn) {
                (*j.fn)(p);
                continue;
            }
            int s = 0;
            while (p >= j.first[s + 1])
                ++s;
            const size_t off = (p - j.first[s]) * kPiece;
            const size_t len = std::min(kPiece, j.seg[s].n - off);
            piece_copy((uint8_t*)j.seg[s].dst + off, (const uint8_t*)j.seg[s].src + off, len);
        }
        if (done && j.finished.fetch_add(done) + done == j.total) {
            std::lock_guard<std::mutex> g(m_);
            done_.notify_all();
        }
    }

    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            Job* j;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (!(j = job_))
                    continue;
                ++j->users;
            }
            work(*j);
            std::lock_guard<std::mutex> g(m_);
            if (--j->users == 0)
                done_.notify_all();
        }
    }

    std::mutex m_;
    std::condition_variable cv_, done_;
    uint64_t gen_ = 0;
    Job* job_ = nullptr;
};

// Set in a forked child (pthread_atfork, registered at load): its copies run single-threaded.
std::atomic<bool> g_fork_child { false };
[[maybe_unused]] const int g_atfork_registered = pthread_atfork(nullptr, nullptr, [] { g_fork_child.store(true); });

inline void par_memcpy_n(const CopySeg* segs, int nseg)
{
    size_t total = 0;
    for (int i = 0; i < nseg; ++i)
        total += segs[i].n;
    if (g_fork_child.load(std::memory_order_relaxed) || copy_threads() == 1 || total < (2u << 20)) {
        for (int i = 0; i < nseg; ++i)
            std::memcpy(segs[i].dst, segs[i].src, segs[i].n);
        return;
    }
    CopyPool::get().run(segs, nseg);
}

inline void par_memcpy(void* dst, const void* src, size_t n)
{
    const CopySeg s { dst, src, n };
    par_memcpy_n(&s, 1);
}

} // namespace
