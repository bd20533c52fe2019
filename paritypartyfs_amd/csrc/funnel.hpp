#pragma once
// funnel.hpp -- 16 bytes at any byte address from aligned dword loads (device code): the read of
// the block-list kernels (vote.hip gather / scatter / extent copy) and of the list decode's row
// fetch (rs_wg_list.hpp), whose sources start at any byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ppfs {

// the 16 bytes at p (any alignment) from aligned dword loads; the caller guarantees that the
// aligned dwords covering [p, p + 16) may be read
__device__ inline uint4 load16_funnel(const uint8_t* p)
{
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* a = (const uint32_t*)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3];
    if (sh == 0)
        return make_uint4(w0, w1, w2, w3);
    const uint32_t w4 = a[4];
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
        __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// the same in two steps, for a loader that issues the loads of many windows before it uses any:
// always the five aligned dwords from the one that holds p[0] (the caller guarantees those 20 bytes)
struct Funnel5 {
    uint32_t w[5];
};
__device__ __forceinline__ Funnel5 funnel_load5(const uint32_t* a)
{
    return Funnel5 { { a[0], a[1], a[2], a[3], a[4] } };
}
__device__ __forceinline__ uint4 funnel_shift(const Funnel5& f, uint32_t sh) // sh = address of byte 0, mod 4
{
    // v_alignbyte with a shift of 0 returns the low dword: no special case
    return make_uint4(__builtin_amdgcn_alignbyte(f.w[1], f.w[0], sh), __builtin_amdgcn_alignbyte(f.w[2], f.w[1], sh),
        __builtin_amdgcn_alignbyte(f.w[3], f.w[2], sh), __builtin_amdgcn_alignbyte(f.w[4], f.w[3], sh));
}

} // namespace ppfs
