// test_resident_plan.cpp -- the resident-prefix plan of the RS 2t <= 8 ticket launches
// (paritypartyfs_amd/csrc/resident_plan.hpp) on the host: the prefix of a batch in tiles and the
// PPFS_ECC_RESIDENT_MIB override.  No HIP: the host compiler alone (tests/test_resident_plan_cpu.py).
#include <cstdint>
#include <cstdio>

#include "../../paritypartyfs_amd/csrc/resident_plan.hpp"

using namespace ppfs::plan;

static int g_fail = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);                                                   \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main()
{
    const uint64_t T = kResidentTileBytes, MIB = 1u << 20;
    CHECK(T == 64u * 255u);
    // a zero-tile batch has no prefix, whatever the setting
    CHECK(resident_tiles(0, 0) == 0);
    CHECK(resident_tiles(0, 192 * MIB) == 0);
    // a batch smaller than the prefix: every tile, the ragged last one included
    CHECK(resident_tiles(1, 192 * MIB) == 1);
    CHECK(resident_tiles(64, 192 * MIB) == 1);
    CHECK(resident_tiles(65, 192 * MIB) == 2);
    CHECK(resident_tiles(64 * 5 + 7, 192 * MIB) == 6);
    CHECK(resident_tiles(64 * 5 + 7, 6 * T) == 6);
    // a batch larger than the prefix: whole tiles that fit the bytes, rounded down
    CHECK(resident_tiles(1u << 20, 192 * MIB) == 192 * MIB / T);
    CHECK(192 * MIB / T == 12336);
    CHECK(resident_tiles(1u << 20, 255 * MIB) == 16384); // 2^20 blocks = 16384 tiles = 255 MiB exactly
    CHECK(resident_tiles((1u << 20) + 1, 255 * MIB) == 16384);
    CHECK(resident_tiles(64 * 5 + 7, 2 * T) == 2);
    CHECK(resident_tiles(64 * 5 + 7, 3 * T - 1) == 2);
    CHECK(resident_tiles(64 * 5 + 7, 3 * T) == 3);
    CHECK(resident_tiles(64 * 5 + 7, T - 1) == 0);
    CHECK(resident_tiles(~0ull, ~0ull) == (~0ull) / T); // no overflow at the ends
    // override 0: the prefix is off
    CHECK(resident_env("0", 192 * MIB) == 0);
    CHECK(resident_env("0.0", 192 * MIB) == 0);
    CHECK(resident_tiles(1u << 20, resident_env("0", 192 * MIB)) == 0);
    // the override in MiB, fractions allowed
    CHECK(resident_env("128", 0) == 128 * MIB);
    CHECK(resident_env("0.5", 0) == MIB / 2);
    CHECK(resident_tiles(64 * 5 + 7, resident_env("0.038909912", 0)) == 2); // 2.5 tiles of bytes
    CHECK(resident_tiles(64 * 5 + 7, resident_env("0.054473877", 0)) == 3); // 3.5 tiles
    CHECK(resident_env("1e30", 0) == (1ull << 40)); // capped at 1 TiB
    // unset, empty, negative, not a number, trailing text: the default
    CHECK(resident_env(nullptr, 7) == 7);
    CHECK(resident_env("", 7) == 7);
    CHECK(resident_env("-1", 7) == 7);
    CHECK(resident_env("abc", 7) == 7);
    CHECK(resident_env("12MiB", 7) == 7);
    CHECK(resident_env("nan", 7) == 7);
    CHECK(resident_env("inf", 7) == 7);
    CHECK(resident_env(nullptr) == kResidentBytesDefault);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
