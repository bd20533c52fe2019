// test_host_plan.cpp -- the host path's arithmetic and CPU copies (paritypartyfs_amd/csrc/host_plan.hpp,
// host_copy.hpp) without a GPU: chunk sizes, staging layout, changed-block scan, patch-list
// application, threaded copies.  Built and run by tests/test_host_plan.py; `copies` as the only
// argument runs the copy checks alone (the driver repeats those under other environments).
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../paritypartyfs_amd/csrc/host_copy.hpp"
#include "../../paritypartyfs_amd/csrc/host_plan.hpp"

using namespace ppfs::plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (++g_fail <= 20) {                                                                                      \
                std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond);                                          \
                std::printf(__VA_ARGS__);                                                                              \
                std::printf("\n");                                                                                     \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static std::vector<size_t> pieces(size_t nblocks, size_t chunk_blocks_)
{
    ChunkSeq seq(nblocks, chunk_blocks_);
    std::vector<size_t> v;
    for (size_t nb; (nb = seq.next()) != 0 && v.size() <= nblocks;)
        v.push_back(nb);
    return v;
}

// The ramp as it was before every piece was bounded by the chunk: the default chunk sizes never
// reached that bound, so for them the sequence must be this one, piece for piece.
static size_t ramp_before(size_t index, size_t remaining, size_t chunk)
{
    const size_t least = std::max<size_t>(chunk / 8, 1024);
    size_t nb = chunk;
    if (index < 3)
        nb = std::max(least, chunk >> (3 - index));
    if (remaining < 2 * nb)
        nb = std::max(least, (remaining / 2 + 1023) & ~(size_t)1023);
    return remaining < nb + least ? remaining : nb;
}

static void check_pieces(size_t nblocks, size_t chunk, bool is_default)
{
    const std::vector<size_t> v = pieces(nblocks, chunk);
    size_t sum = 0, big = 0;
    bool zero = false;
    for (size_t nb : v) {
        sum += nb;
        big = std::max(big, nb);
        zero |= nb == 0;
    }
    CHECK(sum == nblocks, "chunk %zu nblocks %zu: pieces sum to %zu", chunk, nblocks, sum);
    CHECK(!zero, "chunk %zu nblocks %zu: empty piece", chunk, nblocks);
    CHECK(big <= std::min(chunk, nblocks), "chunk %zu nblocks %zu: piece of %zu", chunk, nblocks, big);
    if (nblocks < 8 * chunk) { // chunk, chunk, ..., remainder
        const size_t c = std::min(chunk, nblocks);
        bool ok = v.size() == (nblocks + c - 1) / c;
        for (size_t i = 0; ok && i < v.size(); ++i)
            ok = v[i] == (i + 1 < v.size() ? c : nblocks - c * (v.size() - 1));
        CHECK(ok, "chunk %zu nblocks %zu: not whole chunks and a remainder", chunk, nblocks);
    } else if (is_default) {
        size_t i = 0, b0 = 0;
        bool ok = true;
        for (; b0 < nblocks && i < v.size() && ok; b0 += v[i], ++i)
            ok = v[i] == ramp_before(i, nblocks - b0, chunk);
        CHECK(ok && b0 == nblocks && i == v.size(), "chunk %zu nblocks %zu: piece %zu differs from the ramp", chunk, nblocks, i);
    }
}

static void test_chunk_sizes()
{
    std::set<size_t> defaults;
    for (size_t raw = 1; raw <= 4096; ++raw)
        defaults.insert(chunk_blocks(raw, 0));
    CHECK(chunk_blocks(255, 0) == 65536 && chunk_blocks(4096, 0) == 4096 && *defaults.begin() == 4096,
        "default chunk sizes: %zu %zu %zu", chunk_blocks(255, 0), chunk_blocks(4096, 0), *defaults.begin());
    for (size_t d : defaults)
        CHECK(d % 1024 == 0, "default chunk %zu is no multiple of 1 Ki", d);
    const size_t envs[] = { 1024, 1500, 2048, 3000, 4096, 5000, 8192, 10000, 65536 };
    for (size_t e : envs) {
        char s[32];
        std::snprintf(s, sizeof s, "%zu", e);
        CHECK(chunk_env(s) == e && chunk_blocks(255, chunk_env(s)) == e, "env %zu not taken", e);
    }
    CHECK(chunk_env(nullptr) == 0 && chunk_env("1023") == 0 && chunk_env("4194305") == 0 && chunk_env("x") == 0,
        "out-of-range env values must be ignored");
    std::vector<std::pair<size_t, bool>> chunks;
    for (size_t d : defaults)
        chunks.push_back({ d, true });
    for (size_t e : envs)
        chunks.push_back({ e, defaults.count(e) != 0 });
    std::mt19937_64 rng(20260);
    for (auto [chunk, is_default] : chunks) {
        for (size_t x = 0; x < 3000; ++x)
            check_pieces(8 * chunk + x, chunk, is_default);
        for (int i = 0; i < 3000; ++i)
            check_pieces(1 + rng() % (48 * chunk), chunk, is_default);
    }
}

static void test_chunk_sizes_unchanged()
{
    // from the function as it was (the ramp before the bound), computed by that code itself
    const std::vector<size_t> a = { 8192, 16384, 32768, 65536, 65536, 65536, 65536, 65536, 65536, 44032, 21504, 11264, 9273 };
    CHECK(pieces(8 * 65536 + 12345, chunk_blocks(255, 0)) == a, "chunk 65536, 8 chunks + 12345");
    const std::vector<size_t> b = { 1024, 1024, 2048, 4096, 4096, 4096, 4096, 4096, 4096, 3072, 1801 };
    CHECK(pieces(8 * 4096 + 777, chunk_blocks(4096, 0)) == b, "chunk 4096, 8 chunks + 777");
}

static void test_layout()
{
    struct Cfg {
        const char* name;
        size_t data, raw;
        uint32_t slots;
    };
    const Cfg cfgs[] = { { "RS 512/3", 249, 255, 2 }, { "RS 64/3", 58, 64, 0 }, { "RS 4096/16", 223, 255, 2 },
        { "Hamming 4096", 4091, 4096, 1 }, { "CRC-32 4096", 4092, 4096, 0 }, { "parity 256", 255, 256, 0 } };
    const size_t nbs[] = { 1, 64, 65, 1024, 65536 };
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    for (const Cfg& c : cfgs) {
        size_t prev_total = 0;
        for (size_t nb : nbs) {
            const Layout L = layout_for(c.data, c.raw, c.slots, nb);
            const size_t rows = nb / 8 + 1, spill_b = 256 - std::min<size_t>(c.raw, 255);
            CHECK(spill_bytes(c.raw) == spill_b && gather_rows(nb) == rows && kGatherDiv == 8, "%s: spill / gather sizes", c.name);
            const size_t off[] = { L.data, L.raw, L.status, L.spill, L.idx, L.gat, L.orig, L.patch, L.total };
            const size_t used[] = { nb * c.data, nb * c.raw, nb, nb * spill_b, rows * 4, rows * c.raw,
                c.slots ? nb * c.raw : 0, nb * c.slots * 4 };
            for (int i = 0; i < 9; ++i)
                CHECK(off[i] % 256 == 0, "%s nb %zu: region %d at %zu is not 256-aligned", c.name, nb, i, off[i]);
            for (int i = 0; i < 8; ++i) // in order, each used size ends at or before the next region (and total)
                CHECK(off[i] + used[i] <= off[i + 1], "%s nb %zu: region %d [%zu, +%zu) runs into %zu", c.name, nb, i, off[i],
                    used[i], off[i + 1]);
            CHECK(L.total > prev_total, "%s: total not monotone at nb %zu", c.name, nb);
            prev_total = L.total;
            if (nb <= 64) { // the resident server's layout (server_box.hpp srv_layout): 256-byte rounding
                CHECK(L.data == 0 && L.raw == al(nb * c.data) && L.status == al(al(nb * c.data) + nb * c.raw),
                    "%s nb %zu: differs from the server layout", c.name, nb);
            }
        }
        for (size_t nb = 1; nb < 3000; ++nb)
            CHECK(layout_for(c.data, c.raw, c.slots, nb + 1).total >= layout_for(c.data, c.raw, c.slots, nb).total,
                "%s: total shrinks at nb %zu", c.name, nb);
    }
}

static void test_scan()
{
    const size_t nb = 4096, rows = gather_rows(nb);
    std::mt19937_64 rng(77);
    for (size_t cnt : { nb / 8 - 1, nb / 8, nb / 8 + 1, (size_t)0, nb }) {
        std::vector<uint8_t> sts(nb);
        for (auto& s : sts)
            s = (rng() & 1) ? 0 : 5;
        std::vector<uint32_t> want;
        for (size_t left = cnt; left;) {
            const size_t b = rng() % nb;
            if (sts[b] != 1) {
                sts[b] = 1;
                --left;
            }
        }
        for (size_t b = 0; b < nb; ++b)
            if (sts[b] == 1)
                want.push_back((uint32_t)b);
        std::vector<uint32_t> ix(rows + 4, 0xDEADBEEFu);
        const Changed c = scan_changed(sts.data(), nb, ix.data());
        CHECK(c.count == cnt && c.eager == (cnt > nb / 8), "scan: %zu changed, got %zu eager %d", cnt, c.count, (int)c.eager);
        const size_t listed = std::min(cnt, rows);
        CHECK(std::equal(want.begin(), want.begin() + listed, ix.begin()), "scan: index list at %zu changed", cnt);
        for (size_t i = listed; i < ix.size(); ++i)
            CHECK(ix[i] == 0xDEADBEEFu, "scan: wrote index %zu of %zu rows", i, rows);
        const Changed c0 = scan_changed(sts.data(), nb, nullptr);
        CHECK(c0.count == cnt && c0.eager == c.eager, "scan without a list at %zu changed", cnt);
    }
}

// a patch list for random byte changes: the image before, the image the host must end with (blocks
// that overflow their slots stay as they were: they come back whole), the overflowed blocks
struct PatchCase {
    size_t nb, n;
    uint32_t S;
    std::vector<uint8_t> sts, before, want;
    std::vector<uint32_t> P, over;
};
static PatchCase make_patch_case(size_t nb, size_t n, uint32_t S, uint64_t seed, bool all_changed)
{
    PatchCase t { nb, n, S, std::vector<uint8_t>(nb), std::vector<uint8_t>(nb * n), {}, std::vector<uint32_t>(nb * S), {} };
    std::mt19937_64 rng(seed);
    for (auto& b : t.before)
        b = (uint8_t)rng();
    t.want = t.before;
    const uint8_t kinds[3] = { 0, 1, 5 };
    for (size_t b = 0; b < nb; ++b)
        t.sts[b] = all_changed ? 1 : kinds[rng() % 3];
    if (!all_changed && nb > 16) { // corrected blocks beside uncorrectable ones
        t.sts[10] = 1, t.sts[11] = 5, t.sts[12] = 1, t.sts[13] = 5, t.sts[14] = 0, t.sts[15] = 1;
    }
    for (size_t b = 0; b < nb; ++b) {
        uint32_t* q = &t.P[b * S];
        if (t.sts[b] != 1) { // a list entry the host must not apply: the block did not change
            for (uint32_t j = 0; j < S; ++j)
                q[j] = (uint32_t)((rng() % n) << 8) | 0x5Au;
            continue;
        }
        const uint32_t changes = 1 + (uint32_t)(rng() % (S + 1)); // 1 .. S, or S + 1: overflow
        if (changes > S) {
            q[0] = kPatchOverflow;
            for (uint32_t j = 1; j < S; ++j)
                q[j] = (uint32_t)rng();
            t.over.push_back((uint32_t)b);
            continue;
        }
        std::set<size_t> used;
        for (uint32_t j = 0; j < S; ++j) {
            if (j >= changes) {
                q[j] = kPatchEnd;
                continue;
            }
            size_t off = rng() % n;
            while (used.count(off))
                off = (off + 1) % n;
            used.insert(off);
            const uint8_t v = (uint8_t)(t.before[b * n + off] ^ (1 + rng() % 255));
            q[j] = (uint32_t)(off << 8) | v;
            t.want[b * n + off] = v;
        }
    }
    return t;
}

static void test_patches()
{
    for (uint32_t S : { 1u, 2u }) {
        const PatchCase t = make_patch_case(5000, S == 1 ? 64 : 255, S, 100 + S, false);
        std::vector<uint8_t> img = t.before;
        const std::vector<uint32_t> over = apply_patch_list(img.data(), t.n, t.sts.data(), t.P.data(), S, t.nb, false);
        CHECK(img == t.want, "patch list S %u: image differs", S);
        CHECK(over == t.over && !t.over.empty(), "patch list S %u: overflow list differs (%zu vs %zu)", S, over.size(), t.over.size());
    }
    // pooled against serial: three parts and a bit, every block changed (more than 4 x 4096 changed bytes)
    const PatchCase t = make_patch_case(3 * 4096 + 5, 255, 2, 7, true);
    std::vector<uint8_t> a = t.before, b = t.before;
    const std::vector<uint32_t> oa = apply_patch_list(a.data(), t.n, t.sts.data(), t.P.data(), t.S, t.nb, false);
    const std::vector<uint32_t> ob = apply_patch_list(b.data(), t.n, t.sts.data(), t.P.data(), t.S, t.nb, true);
    CHECK(a == t.want && b == t.want, "pooled / serial patch application: image differs");
    CHECK(oa == t.over && ob == t.over, "pooled / serial patch application: overflow list differs");
    CHECK(!patch_pooled(4096, 1u << 20) && !patch_pooled(1u << 20, 4 * 4096), "pool threshold");
}

static void test_copies()
{
    const size_t n0 = (3u << 20) + 1, n1 = (2u << 20) - 7, guard = 256;
    std::mt19937_64 rng(5);
    std::vector<uint8_t> src(n0 + n1 + 64), dst(n0 + n1 + 4 * guard + 64, 0xC3);
    for (auto& b : src)
        b = (uint8_t)rng();
    // unaligned on both sides; the segments' destinations are `guard` bytes apart
    const uint8_t *s0 = src.data() + 3, *s1 = src.data() + 3 + n0 + 10;
    uint8_t *d0 = dst.data() + guard + 5, *d1 = d0 + n0 + guard + 3;
    const CopySeg segs[2] = { { d0, s0, n0 }, { d1, s1, n1 } };
    par_memcpy_n(segs, 2);
    CHECK(std::memcmp(d0, s0, n0) == 0 && std::memcmp(d1, s1, n1) == 0, "par_memcpy_n: bytes differ");
    std::vector<uint8_t> want(dst.size(), 0xC3);
    std::memcpy(want.data() + (d0 - dst.data()), s0, n0);
    std::memcpy(want.data() + (d1 - dst.data()), s1, n1);
    CHECK(dst == want, "par_memcpy_n: wrote outside its destinations");
    std::vector<uint8_t> one(n0 + 2 * guard, 0x3C), one_want(n0 + 2 * guard, 0x3C);
    par_memcpy(one.data() + guard + 1, s0, n0 - 1);
    std::memcpy(one_want.data() + guard + 1, s0, n0 - 1);
    CHECK(one == one_want, "par_memcpy: bytes or guards differ");
}

int main(int argc, char** argv)
{
    const bool copies_only = argc > 1 && std::strcmp(argv[1], "copies") == 0;
    if (!copies_only) {
        test_chunk_sizes();
        test_chunk_sizes_unchanged();
        test_layout();
        test_scan();
        test_patches();
    }
    test_copies();
    if (g_fail) {
        std::printf("%d check(s) FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED (copy threads %d)\n", copy_threads());
    return 0;
}
