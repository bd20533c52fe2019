// test_alloc_plan.cpp -- the arithmetic of the allocated-block scrub (paritypartyfs_amd/csrc/alloc_plan.hpp)
// on the host, against a bit-by-bit restatement of the reference's Bitmap::getBit (lib/bitmap/src/
// bitmap.cpp:8-14, 98-100): the word transform, the tail mask, the failed-block mask, the blocks spanned,
// the piece cut, and an emulation of the three kernels of alloc_scan.hip (count, offsets, expand) with
// their chunking, which must yield exactly the ascending list of set bits and its length.  The payload
// stream is a heap buffer of exactly B * dataSize() bytes, so the address sanitizer sees any read past
// it; every read is also checked by hand.  No HIP: built with the host compiler (tests/test_alloc_cpu.py,
// with the address and undefined-behaviour sanitizers).
#include "../../paritypartyfs_amd/csrc/alloc_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ppfs::alloc;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail < 20)                                                                                           \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// the decoded bitmap as the plan reads it; every read checked against the stream's and the statuses' ends
struct Src {
    const uint8_t* stream;
    uint64_t stream_bytes;
    const uint8_t* bstatus;
    uint64_t B;
    uint32_t dword(uint64_t w) const
    {
        CHECK(4 * w + 4 <= stream_bytes);
        const uint8_t* p = stream + 4 * w;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    uint32_t byte(uint64_t i) const
    {
        CHECK(i < stream_bytes);
        return stream[i];
    }
    uint32_t status(uint64_t b) const
    {
        CHECK(b < B);
        return bstatus[b];
    }
};

// Bitmap::getBit restated: byte j / 8 of the stream under mask 0x80 >> (j % 8)
static bool get_bit(const uint8_t* stream, uint64_t j) { return (stream[j / 8] & (0x80u >> (j % 8))) != 0; }

// the scrub's rule on top: a failed bitmap block's bits count as set
static bool want_bit(const uint8_t* stream, const uint8_t* bstatus, uint64_t ds, uint64_t j)
{
    return bstatus[j / (8 * ds)] == 5 || get_bit(stream, j);
}

// count / offsets / expand as alloc_scan.hip runs them: per piece, one "workgroup" of CHUNK_WORDS lanes
// per chunk, a lane's slot = its chunk's offset + the exclusive prefix of the lanes before it
static std::vector<uint32_t> emulate(const Src& src, uint64_t nbits, uint64_t ds, uint32_t first_block, uint64_t* total_out)
{
    std::vector<uint32_t> list;
    uint64_t total = 0;
    for (uint64_t p = 0; p < pieces_of(nbits); ++p) {
        const Piece pc = piece_of(nbits, p);
        CHECK(pc.chunks >= 1 && pc.chunks <= PIECE_CHUNKS && pc.word0 * 32 == pc.bit0);
        uint32_t tot[PIECE_CHUNKS], off[PIECE_CHUNKS];
        for (uint32_t ch = 0; ch < pc.chunks; ++ch) { // alloc_count_kernel
            tot[ch] = 0;
            for (uint32_t lane = 0; lane < CHUNK_WORDS; ++lane)
                tot[ch] += (uint32_t)__builtin_popcount(word_bits(src, pc.word0 + (uint64_t)ch * CHUNK_WORDS + lane, nbits, ds, src.B));
        }
        uint32_t piece_total = 0;
        for (uint32_t ch = 0; ch < pc.chunks; ++ch) { // alloc_offsets_kernel
            off[ch] = piece_total;
            piece_total += tot[ch];
        }
        CHECK(piece_total <= pc.bits);
        std::vector<uint32_t> index(piece_total, 0xFFFFFFFFu);
        for (uint32_t ch = 0; ch < pc.chunks; ++ch) { // alloc_expand_kernel
            uint32_t prefix = 0;
            for (uint32_t lane = 0; lane < CHUNK_WORDS; ++lane) {
                const uint64_t w = pc.word0 + (uint64_t)ch * CHUNK_WORDS + lane;
                uint32_t bits = word_bits(src, w, nbits, ds, src.B);
                uint32_t at = off[ch] + prefix;
                prefix += (uint32_t)__builtin_popcount(bits);
                const uint32_t base = first_block + (uint32_t)(32 * w);
                for (; bits; bits &= bits - 1, ++at) {
                    CHECK(at < piece_total);
                    if (at < piece_total)
                        index[at] = base + (uint32_t)__builtin_ctz(bits);
                }
            }
        }
        list.insert(list.end(), index.begin(), index.end());
        total += piece_total;
    }
    *total_out = total;
    return list;
}

static uint32_t g_seed = 12345;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

static void fill(uint8_t* s, uint64_t n, int pattern)
{
    for (uint64_t i = 0; i < n; ++i)
        s[i] = pattern == 0 ? 0x00 : pattern == 1 ? 0xFF : pattern == 2 ? 0xAA : (uint8_t)(rnd() >> 24);
}

static void run_case(uint64_t ds, uint64_t nbits, int pattern, long failed /* -1: none */)
{
    const uint64_t B = blocks_spanned(nbits, ds), stream_bytes = B * ds, bpb = 8 * ds;
    uint8_t* stream = (uint8_t*)std::malloc(stream_bytes); // exactly the stream: a read past it is a sanitizer report
    std::vector<uint8_t> bstatus(B, 0);
    fill(stream, stream_bytes, pattern);
    if (failed >= 0)
        bstatus[(size_t)failed] = 5;
    if (B > 1 && failed != 0)
        bstatus[0] = 1; // a corrected block's bits are its payload's
    const Src src { stream, stream_bytes, bstatus.data(), B };
    const uint32_t first_block = 1000;

    std::vector<uint32_t> want;
    for (uint64_t j = 0; j < nbits; ++j)
        if (want_bit(stream, bstatus.data(), ds, j))
            want.push_back(first_block + (uint32_t)j);

    for (uint64_t w = 0; w < words_of(nbits) + 2; ++w) { // two words past the end as well: they must be empty
        const uint32_t got = word_bits(src, w, nbits, ds, B);
        uint32_t exp = 0, tail = 0, fm = 0;
        for (uint32_t i = 0; i < 32; ++i) {
            const uint64_t j = 32 * w + i;
            if (j < nbits) {
                tail |= 1u << i;
                if (want_bit(stream, bstatus.data(), ds, j))
                    exp |= 1u << i;
            }
            if (j / bpb < B && bstatus[j / bpb] == 5)
                fm |= 1u << i;
        }
        CHECK(got == exp);
        CHECK(tail_mask(w, nbits) == tail);
        CHECK(failed_mask(src, w, bpb, B) == fm);
        const uint64_t at = 4 * w;
        CHECK(word_bytes(w, stream_bytes) == (at >= stream_bytes ? 0u : (uint32_t)(stream_bytes - at < 4 ? stream_bytes - at : 4)));
    }
    uint64_t total = 0;
    const std::vector<uint32_t> got = emulate(src, nbits, ds, first_block, &total);
    CHECK(total == want.size());
    CHECK(got == want);
    std::free(stream);
}

int main()
{
    // the word transform: bit i of the result is stream bit i (byte i / 8 under mask 0x80 >> (i % 8))
    for (int k = 0; k < 2000; ++k) {
        const uint32_t le = k < 32 ? 1u << k : rnd();
        const uint8_t bytes[4] = { (uint8_t)le, (uint8_t)(le >> 8), (uint8_t)(le >> 16), (uint8_t)(le >> 24) };
        uint32_t exp = 0;
        for (uint32_t i = 0; i < 32; ++i)
            if (get_bit(bytes, i))
                exp |= 1u << i;
        CHECK(stream_bits(le) == exp);
    }

    const uint64_t sizes[] = { 1, 3, 58, 249, 4080 };
    const uint64_t bits[] = { 1, 7, 8, 9, 31, 32, 33, 1991, 1992, 1993, 8191, 8192, 8193 };
    long cases = 0;
    for (uint64_t ds : sizes)
        for (uint64_t nbits : bits) {
            // Bitmap::blocksSpanned (bitmap.cpp:27-31), the reference's floating-point form in double
            const uint64_t B = blocks_spanned(nbits, ds);
            CHECK(B == (uint64_t)std::ceil(std::ceil((double)nbits / 8.0) / (double)ds));
            CHECK(B * ds * 8 >= nbits && (B - 1) * ds * 8 < nbits);
            for (int pattern = 0; pattern < 4; ++pattern)
                for (long failed = -1; failed < (long)B; ++failed, ++cases)
                    run_case(ds, nbits, pattern, failed);
        }

    // the piece cut: a range of more than one piece, the second piece short and ragged
    {
        const uint64_t nbits = PIECE_BITS + 8197;
        CHECK(pieces_of(nbits) == 2 && pieces_of(PIECE_BITS) == 1 && pieces_of(PIECE_BITS + 1) == 2 && pieces_of(1) == 1);
        const Piece a = piece_of(nbits, 0), b = piece_of(nbits, 1);
        CHECK(a.bit0 == 0 && a.bits == PIECE_BITS && a.word0 == 0 && a.chunks == PIECE_CHUNKS);
        CHECK(b.bit0 == PIECE_BITS && b.bits == 8197 && b.word0 == PIECE_WORDS && b.chunks == 2);
        run_case(58, nbits, 3, 7);
        run_case(58, nbits, 3, (long)blocks_spanned(nbits, 58) - 1);
        cases += 2;
    }

    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED (%ld cases)\n", cases);
    return 0;
}
