// host_tables.hpp -- host builders of the codec tables the kernels read: GF(2^8) log / antilog, the
// RS slicing / workgroup / pair tables (layouts: rs_layout.hpp, emission schedule: rs_sched.hpp) and
// the CRC shift tables.  Plain C++: the engine (api.cpp) and the probes under tools/probes include
// it; the only kernel-side functions it needs are the three sizing functions declared below.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "rs_layout.hpp"
#include "rs_sched.hpp"

extern "C" {
int ppfs_rs_fast_tables_bytes(int t2); // rs_kernels.hip
int ppfs_crc_tables_bytes(void); // bit_kernels.hip
int ppfs_crc_fast_layout(int32_t* v, int n); // bit_fast.hip
}

namespace {

// ---------------------------------------------------------------------------------------
// GF(2^8) host tables (gf256.cpp:6-29)
// ---------------------------------------------------------------------------------------
struct GfHost {
    uint8_t exp[256], log[256];
    GfHost()
    {
        unsigned x = 1;
        for (int i = 0; i < 255; ++i) {
            exp[i] = (uint8_t)x;
            x <<= 1;
            if (x & 0x100)
                x ^= 0x11D;
        }
        exp[255] = exp[0];
        std::memset(log, 0, sizeof log);
        for (int i = 0; i < 255; ++i)
            log[exp[i]] = (uint8_t)i;
    }
    uint8_t mul(uint8_t a, uint8_t b) const
    {
        if (!a || !b)
            return 0;
        return exp[(log[a] + log[b]) % 255];
    }
};
inline const GfHost& gf()
{
    static GfHost g;
    return g;
}

// 1 KiB block: EXP2[512] | LOG[256] | QS[256]
inline void build_gf_block(uint8_t* out)
{
    const GfHost& g = gf();
    for (int i = 0; i < 512; ++i)
        out[i] = g.exp[i % 255];
    std::memcpy(out + 512, g.log, 256);
    uint8_t* qs = out + 768;
    std::memset(qs, 0, 256);
    for (int y = 2; y < 256; ++y) {
        const uint8_t c = (uint8_t)(g.mul((uint8_t)y, (uint8_t)y) ^ y);
        if (!qs[c])
            qs[c] = (uint8_t)y;
    }
}

// generator g(x) = prod_{i=1..2t}(x + alpha^i), low -> high (rs_block_device.cpp:195-208)
inline std::vector<uint8_t> rs_generator(int t2)
{
    const GfHost& G = gf();
    std::vector<uint8_t> g(1, 1);
    uint8_t power = 2;
    for (int i = 0; i < t2; ++i) {
        std::vector<uint8_t> ng(g.size() + 1, 0);
        for (size_t k = 0; k < g.size(); ++k) {
            ng[k] ^= G.mul(g[k], power);
            ng[k + 1] ^= g[k];
        }
        g.swap(ng);
        power = G.mul(power, 2);
    }
    return g;
}

// x^e mod g (monic, degree t2): returns t2 coefficients
inline std::vector<uint8_t> rs_xpow_mod(int e, const std::vector<uint8_t>& g, int t2)
{
    const GfHost& G = gf();
    std::vector<uint8_t> r(t2, 0);
    r[0] = 1;
    if (t2 == 0)
        return r;
    for (int k = 0; k < e; ++k) {
        const uint8_t top = r[t2 - 1];
        for (int q = t2 - 1; q >= 1; --q)
            r[q] = (uint8_t)(r[q - 1] ^ G.mul(top, g[q]));
        r[0] = G.mul(top, g[0]);
    }
    return r;
}

// slicing tables for the fast path (see rs_kernels.hip: slice8)
inline std::vector<uint8_t> build_rs_slice_tables(int t2)
{
    const GfHost& G = gf();
    const int W = t2 <= 8 ? 2 : (t2 <= 16 ? 4 : 8);
    const int bytes = ppfs_rs_fast_tables_bytes(t2);
    std::vector<uint8_t> out((size_t)bytes, 0);
    const std::vector<uint8_t> g = rs_generator(t2);
    for (int i = 0; i < 8; ++i) {
        const std::vector<uint8_t> xi = rs_xpow_mod(t2 + i, g, t2);
        for (int h = 0; h < 2; ++h) {
            for (int v = 0; v < 16; ++v) {
                const uint8_t val = (uint8_t)(v << (4 * h));
                uint8_t entry[32] = { 0 };
                for (int q = 0; q < t2; ++q)
                    entry[4 * W - t2 + q] = G.mul(val, xi[q]);
                const size_t slot = (size_t)((2 * i + h) * 16 + v) * 16;
                if (W <= 4) {
                    std::memcpy(&out[slot], entry, (size_t)(4 * W));
                } else {
                    std::memcpy(&out[slot], entry, 16);
                    std::memcpy(&out[4096 + slot], entry + 16, 16);
                }
            }
        }
    }
    return out;
}

// tables of the workgroup-cooperative RS path, 2t <= 8 (layout: rs_layout.hpp)
template <int T2> inline std::vector<uint8_t> build_rs_wg_tables_t()
{
    using L = ppfs::RsWgLayout<T2>;
    const GfHost& G = gf();
    std::vector<uint8_t> out((size_t)L::BLOB_BYTES, 0);
    const std::vector<uint8_t> g = rs_generator(T2);
    // top-aligned 8-byte entry of a remainder r (coefficient q at byte 8 - 2t + q)
    auto put = [&](int off, int table, int v, const std::vector<uint8_t>& r, uint8_t scale) {
        for (int q = 0; q < T2; ++q)
            out[(size_t)off + (size_t)table * L::TBL + (size_t)v * L::ES + (8 - T2 + q)] = G.mul(scale, r[q]);
    };
    for (int i = 0; i < 8; ++i) {
        const std::vector<uint8_t> xi = rs_xpow_mod(T2 + i, g, T2);
        for (int h = 0; h < 2; ++h)
            for (int v = 0; v < 16; ++v)
                put(L::OFF_SL, 2 * i + h, v, xi, (uint8_t)(v << (4 * h)));
    }
    for (int m = 0; m < 3; ++m)
        for (int q = 0; q < T2; ++q) {
            const std::vector<uint8_t> xq = rs_xpow_mod(q + 64 * (m + 1), g, T2);
            for (int h = 0; h < 2; ++h)
                for (int v = 0; v < 16; ++v)
                    put(L::OFF_MAP + m * L::MAP_STRIDE, 2 * q + h, v, xq, (uint8_t)(v << (4 * h)));
        }
    for (int m = 0; m < 7; ++m)
        for (int q = 0; q < T2; ++q) {
            const std::vector<uint8_t> xq = rs_xpow_mod(q + 32 * (m + 1), g, T2);
            for (int h = 0; h < 2; ++h)
                for (int v = 0; v < 16; ++v)
                    put(L::OFF_MAP32 + m * L::MAP_STRIDE, 2 * q + h, v, xq, (uint8_t)(v << (4 * h)));
        }
    for (int m = 1; m <= 3; ++m)
        for (int i = 0; i < 8; ++i) {
            const std::vector<uint8_t> xi = rs_xpow_mod(T2 + i + 64 * m, g, T2);
            for (int h = 0; h < 2; ++h)
                for (int v = 0; v < 16; ++v)
                    put(L::OFF_SLX + (m - 1) * 16 * L::TBL, 2 * i + h, v, xi, (uint8_t)(v << (4 * h)));
        }
    for (int q = 0; q < T2; ++q)
        for (int h = 0; h < 2; ++h)
            for (int v = 0; v < 16; ++v)
                for (int i = 1; i <= T2; ++i) {
                    const int e = ((i * (q - T2)) % 255 + 255) % 255;
                    out[(size_t)L::OFF_SYN + (size_t)(2 * q + h) * L::TBL + (size_t)v * L::ES + (i - 1)] =
                        G.mul((uint8_t)(v << (4 * h)), G.exp[e]);
                }
    build_gf_block(out.data() + L::OFF_GF);
    const std::vector<uint16_t> es = ppfs::sched::build_encode(T2);
    std::memcpy(out.data() + L::OFF_ESCHED, es.data(), es.size() * sizeof(uint16_t));
    const std::vector<uint8_t> rm = ppfs::sched::row_map(L::K);
    std::memcpy(out.data() + L::OFF_ROWMAP, rm.data(), rm.size());
    // SL5 / SLX5 from the nibble tables by linearity: bit m of the 64-bit chunk (byte m / 8, nibble
    // half (m % 8) / 4, bit m % 4) contributes nibble table 2 (m / 8) + (m % 8) / 4, entry 1 << (m % 4)
    auto five = [&](int nib_off, int five_off) {
        for (int i = 0; i < 13; ++i)
            for (int v = 0; v < 32; ++v)
                for (int k = 0; k < 5; ++k) {
                    const int m = 5 * i + k;
                    if (!(v >> k & 1) || m >= 64)
                        continue;
                    const size_t src = (size_t)nib_off + (size_t)(2 * (m / 8) + (m % 8) / 4) * L::TBL + (size_t)(1 << (m % 4)) * L::ES;
                    const size_t dst = (size_t)five_off + (size_t)i * 32 * L::ES + (size_t)v * L::ES;
                    for (int b = 0; b < L::ES; ++b)
                        out[dst + (size_t)b] ^= out[src + (size_t)b];
                }
    };
    five(L::OFF_SL, L::OFF_SL5);
    for (int m = 0; m < 3; ++m)
        five(L::OFF_SLX + m * 16 * L::TBL, L::OFF_SLX5 + m * L::SL5_BYTES);
    return out;
}

// tables of the pair RS path, 16 < 2t <= 32 (layout: rs_layout.hpp RsPairLayout)
inline std::vector<uint8_t> build_rs_pair_tables(int t2)
{
    const GfHost& G = gf();
    std::vector<uint8_t> out((size_t)ppfs::rs_pair_table_bytes(), 0);
    const std::vector<uint8_t> g = rs_generator(t2);
    for (int i = 0; i < 8; ++i) {
        const std::vector<uint8_t> xi = rs_xpow_mod(t2 + i, g, t2);
        for (int h = 0; h < 2; ++h)
            for (int v = 0; v < 16; ++v) {
                uint8_t entry[32] = { 0 };
                for (int q = 0; q < t2; ++q)
                    entry[32 - t2 + q] = G.mul((uint8_t)(v << (4 * h)), xi[q]);
                for (int c = 0; c < 2; ++c)
                    std::memcpy(&out[(size_t)(2 * i + h) * 512 + (size_t)c * 256 + (size_t)v * 16], entry + 16 * c, 16);
            }
    }
    build_gf_block(out.data() + 16 * 512);
    uint8_t* xp = out.data() + 16 * 512 + 1024;
    std::memset(xp, 0xFF, 255 * 32);
    for (int p = 0; p < 255; ++p) {
        const std::vector<uint8_t> xr = rs_xpow_mod(p + t2, g, t2);
        for (int q = 0; q < t2; ++q)
            if (xr[q])
                xp[p * 32 + (32 - t2 + q)] = G.log[xr[q]];
    }
    // the same rows for x^p mod g: the single-error check on c mod g (rs_pair.hpp, RM decode)
    uint8_t* xpm = xp + 255 * 32;
    std::memset(xpm, 0xFF, 255 * 32);
    for (int p = 0; p < 255; ++p) {
        const std::vector<uint8_t> xr = rs_xpow_mod(p, g, t2);
        for (int q = 0; q < t2; ++q)
            if (xr[q])
                xpm[p * 32 + (32 - t2 + q)] = G.log[xr[q]];
    }
    // byte-slice tables (rs_bs.hpp): by linearity, byte v at chunk position q maps to the XOR of
    // its two nibble entries; row v, slot 2q + c
    uint8_t* bs = xpm + 255 * 32;
    for (int v = 0; v < 256; ++v)
        for (int q = 0; q < 8; ++q)
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < 16; ++k)
                    bs[v * 256 + (2 * q + c) * 16 + k] = out[(size_t)(2 * q) * 512 + (size_t)c * 256 + (size_t)(v & 15) * 16 + k]
                        ^ out[(size_t)(2 * q + 1) * 512 + (size_t)c * 256 + (size_t)(v >> 4) * 16 + k];
    // S_1, S_2 contributions of the c mod g state bytes (rs_bs.hpp bs_correct; coefficient q of
    // the state is byte 32 - 2t + q, exponent i q)
    uint8_t* s12 = bs + 256 * 256;
    for (int u = 0; u < 32; ++u) {
        const int q = u - (32 - t2);
        for (int v = 0; v < 256; ++v) {
            if (q < 0)
                continue;
            s12[u * 512 + 2 * v] = G.mul((uint8_t)v, G.exp[q % 255]);
            s12[u * 512 + 2 * v + 1] = G.mul((uint8_t)v, G.exp[(2 * q) % 255]);
        }
    }
    return out;
}

inline std::vector<uint8_t> build_rs_fast_tables_uncached(int t2)
{
    if (t2 > 16)
        return build_rs_pair_tables(t2);
    switch (t2) {
    case 2:
        return build_rs_wg_tables_t<2>();
    case 4:
        return build_rs_wg_tables_t<4>();
    case 6:
        return build_rs_wg_tables_t<6>();
    case 8:
        return build_rs_wg_tables_t<8>();
    default: {
        std::vector<uint8_t> s = build_rs_slice_tables(t2);
        s.resize(s.size() + 1024);
        build_gf_block(s.data() + s.size() - 1024);
        return s;
    }
    }
}

// the blob depends on 2t only; built once per process (the emission schedule search of the t <= 4
// layouts takes tens of ms)
inline std::vector<uint8_t> build_rs_fast_tables(int t2)
{
    static std::mutex mu;
    static std::map<int, std::vector<uint8_t>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(t2);
    if (it == cache.end())
        it = cache.emplace(t2, build_rs_fast_tables_uncached(t2)).first;
    return it->second;
}

// ---------------------------------------------------------------------------------------
// CRC host maths over GF(2)[x] / P  (P explicit, degree n <= 63)
// ---------------------------------------------------------------------------------------
struct CrcHost {
    uint64_t P;
    int n;
    uint64_t mask;
    uint64_t mod(uint64_t a) const // reduce a polynomial of degree <= 63
    {
        for (int k = 63; k >= n; --k)
            if ((a >> k) & 1u)
                a ^= P << (k - n);
        return a;
    }
    uint64_t mulx(uint64_t a) const
    {
        const bool top = (a >> (n - 1)) & 1u;
        a = (a << 1) & mask;
        return top ? a ^ (P & mask) : a;
    }
    uint64_t mul(uint64_t a, uint64_t b) const // a*b mod P (a, b reduced)
    {
        uint64_t r = 0;
        for (int k = n - 1; k >= 0; --k) {
            r = mulx(r);
            if ((b >> k) & 1u)
                r ^= a;
        }
        return r;
    }
    uint64_t xpow(long e) const // x^e mod P, e may be negative (x is invertible: P(0) = 1)
    {
        uint64_t base = e >= 0 ? mod(2u) : (P >> 1); // x or x^-1 = (P - 1)/x
        if (e < 0)
            e = -e;
        uint64_t r = mod(1u);
        while (e) {
            if (e & 1)
                r = mul(r, base);
            base = mul(base, base);
            e >>= 1;
        }
        return r;
    }
};

inline std::vector<uint8_t> build_crc_tables(uint64_t P, int n, uint32_t ds)
{
    CrcHost c { P, n, n == 64 ? ~0ull : ((1ull << n) - 1) };
    const uint32_t G = (ds + 63) / 64;
    const long z = 64L * G - ds;
    std::vector<uint8_t> out((size_t)ppfs_crc_tables_bytes(), 0);
    uint64_t* pt = (uint64_t*)out.data();
    for (int pos = 0; pos < 64; ++pos) {
        const uint64_t f = c.xpow(8L * (63 - pos) + n - 8 * z - 1);
        for (int h = 0; h < 2; ++h)
            for (int v = 0; v < 16; ++v)
                pt[(pos * 2 + h) * 16 + v] = c.mul(c.mod((uint64_t)v << (4 * h)), f);
    }
    uint64_t* lv = (uint64_t*)(out.data() + 64 * 2 * 16 * 8);
    for (int j = 0; j < 6; ++j) {
        const uint64_t f = c.xpow(512L << j);
        for (int k = 0; k < 16; ++k)
            for (int v = 0; v < 16; ++v)
                lv[(j * 16 + k) * 16 + v] = (4 * k < 64) ? c.mul(c.mod((uint64_t)v << (4 * k)), f) : 0;
    }
    return out;
}

// Maps of the CRC fast path (bit_fast.hip, n <= 32), at the offsets bit_fast.hip reports
// (ppfs_crc_fast_layout): nibble maps (8 nibble tables x 16 u32 entries, T[i][v] = (v << 4i) * C mod
// P for a constant C = x^e mod P): x^0, x^32, x^64, x^96 (piece dwords), x^8192 (one lane's pieces,
// 1 KiB apart), x^(128 2^j) j < 6 (lane tree; the kernels use j = 4, 5 after the lane maps), the
// encode's placement factors x^(8 (ds + m - 1024 (NP + 1)) + n - 1) for each payload misalignment
// m < 16 and the check's x^(8 (ds - bs) + n - 1); the 16 transposed lane maps; the 6-bit tree maps;
// the 8-bit piece / Horner maps.
inline std::vector<uint8_t> build_crc_fast_tables(uint64_t P, int n, uint32_t ds, uint32_t bs)
{
    struct Lay {
        int32_t map, nmaps, lane_off, lanes, six_off, nsix, map6, eight_off, neight, eight, bytes;
    } ly;
    if (ppfs_crc_fast_layout((int32_t*)&ly, (int)(sizeof(ly) / 4)) != (int)(sizeof(ly) / 4) || ly.map != 8 * 16 * 4
        || ly.lane_off < ly.nmaps * ly.map || ly.six_off < ly.lane_off + ly.lanes * ly.map
        || ly.eight_off < ly.six_off + ly.nsix * ly.map6 || ly.bytes < ly.eight_off + ly.neight * ly.eight || ly.neight != 5
        || ly.nsix != 2 || ly.map6 < 5 * 256 + 16 || ly.eight != 4096)
        return {}; // the device layout changed under this builder: refuse (create fails) rather than misplace
    CrcHost c { P, n, n == 64 ? ~0ull : ((1ull << n) - 1) };
    const long NP = bs / 1024;
    std::vector<long> ex = { 0, 32, 64, 96, 8192 };
    for (int j = 0; j < 6; ++j)
        ex.push_back(128L << j);
    for (long m = 0; m < 16; ++m)
        ex.push_back(8L * ((long)ds + m - 1024L * (NP + 1)) + n - 1);
    ex.push_back(8L * ((long)ds - (long)bs) + n - 1);
    if ((int)ex.size() != ly.nmaps)
        return {};

    std::vector<uint8_t> out((size_t)ly.bytes, 0);
    auto nibble_map = [&](uint8_t* dst, long e) {
        const uint64_t C = c.xpow(e);
        uint32_t* t = (uint32_t*)dst;
        for (int i = 0; i < 8; ++i)
            for (int v = 0; v < 16; ++v)
                t[i * 16 + v] = (uint32_t)c.mul(c.mod((uint64_t)v << (4 * i)), C);
    };
    for (size_t mi = 0; mi < ex.size(); ++mi)
        nibble_map(out.data() + mi * ly.map, ex[mi]);
    // lane maps: lane b of NL = 16 multiplies by x^(128 (NL - 1 - b)), transposed: dword (16 i + v) NL + b
    const int NL = ly.lanes;
    uint32_t* lt = (uint32_t*)(out.data() + ly.lane_off);
    for (int b = 0; b < NL; ++b) {
        const uint64_t C = c.xpow(128L * (NL - 1 - b));
        for (int i = 0; i < 8; ++i)
            for (int v = 0; v < 16; ++v)
                lt[(16 * i + v) * NL + b] = (uint32_t)c.mul(c.mod((uint64_t)v << (4 * i)), C);
    }
    // 6-bit tables of the lane-tree maps x^2048, x^4096 (bit_fast.hip CF_MAP6): sub-table j < 5 = 64
    // entries (v << 6j) C, then 4 entries (v << 30) C
    for (int q = 0; q < 2; ++q) {
        const uint64_t C = c.xpow(ex[9 + q]);
        uint32_t* e = (uint32_t*)(out.data() + ly.six_off + q * ly.map6);
        for (int j = 0; j < 5; ++j)
            for (int v = 0; v < 64; ++v)
                e[64 * j + v] = (uint32_t)c.mul(c.mod((uint64_t)v << (6 * j)), C);
        for (int v = 0; v < 4; ++v)
            e[320 + v] = (uint32_t)c.mul(c.mod((uint64_t)v << 30), C);
    }
    // 8-bit tables (bit_fast.hip CF_EIGHT): x^0, x^32, x^64, x^96 indexed by the bytes of the payload
    // dword in memory order (table k = byte 3 - k of the value), x^8192 by the bytes of a value
    uint32_t* e8 = (uint32_t*)(out.data() + ly.eight_off);
    for (int q = 0; q < 5; ++q) {
        const uint64_t C = c.xpow(ex[q]);
        for (int k = 0; k < 4; ++k) {
            const int vb = q < 4 ? 3 - k : k; // the value byte that input byte k holds
            for (int v = 0; v < 256; ++v)
                e8[q * 1024 + k * 256 + v] = (uint32_t)c.mul(c.mod((uint64_t)v << (8 * vb)), C);
        }
    }
    return out;
}

inline int bitlen64(uint64_t v)
{
    int c = 0;
    while (v) {
        v >>= 1;
        c++;
    }
    return c;
}

} // namespace
