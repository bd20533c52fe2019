#pragma once
// alloc_plan.hpp -- the arithmetic of the allocated-block scrub (scrub_path.cpp, alloc_scan.hip): how
// the reference's on-disk allocation bitmap (lib/bitmap/src/bitmap.cpp) becomes an ascending list of
// block indices.  Plain arithmetic for host and device alike, so the kernels, the host form and
// tests/cpp/test_alloc_plan.cpp (the same plan over a heap buffer, under the address sanitizer)
// decide identically.
//
// The bitmap of nbits bits lies in B = blocks_spanned(nbits, ds) blocks of ds payload bytes each; its
// payload STREAM is those payloads back to back, B * ds bytes.  Bit j is byte j / 8 of the stream
// under mask 0x80 >> (j % 8) (Bitmap::getBit, bitmap.cpp:8-14, 98-100) and stands for image block
// first_block + j.  The stream is consumed in WORDS of 32 bits: word w is stream bytes 4w .. 4w + 3,
// turned by stream_bits() into a word whose bit i is stream bit 32 w + i, so that popcount and
// lowest-set-bit walk the blocks in ascending order.  The last word may be cut short by the stream's
// end: the bytes past it are never read and count as zero.
//
// Two masks apply to a word: tail_mask clears the bits at or past nbits, failed_mask SETS the bits of
// every bitmap block whose decode failed (status 5: its payload is undefined, so every block it
// covers is scrubbed).  A bitmap block covers 8 * ds bits, so its boundaries fall on byte, not on
// word boundaries: a word may lie across up to four blocks (ds = 1).
//
// The cut: the bit range runs in PIECES of PIECE_BITS bits (bounds the list scratch), a piece in
// CHUNKS of CHUNK_WORDS words, one workgroup of CHUNK_WORDS lanes each: count (a chunk's popcount),
// offsets (exclusive scan of a piece's chunk totals), expand (each lane writes its word's blocks).
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace alloc {

constexpr uint64_t PIECE_BITS = 1ull << 20;
constexpr uint32_t CHUNK_WORDS = 256, CHUNK_BITS = 32u * CHUNK_WORDS;         // 8,192 bits per workgroup
constexpr uint32_t PIECE_WORDS = (uint32_t)(PIECE_BITS / 32u);                // 32,768
constexpr uint32_t PIECE_CHUNKS = (uint32_t)(PIECE_BITS / CHUNK_BITS);        // 128
constexpr uint8_t STATUS_FAILED = 5;                                          // PPFS_ECC_CORRECTION_ERROR

// Bitmap::blocksSpanned (bitmap.cpp:27-31): ceil(ceil(nbits / 8) / ds).  The reference computes this
// in float, which is exact only while the byte count has at most 24 significant bits; here it is
// integer arithmetic.  ds > 0.
PPFS_HD inline uint64_t blocks_spanned(uint64_t nbits, uint64_t ds)
{
    const uint64_t bytes = (nbits + 7u) / 8u;
    return (bytes + ds - 1u) / ds;
}

PPFS_HD inline uint64_t words_of(uint64_t nbits) { return (nbits + 31u) / 32u; }

// the little-endian dword of four stream bytes -> the word whose bit i is stream bit i: the bits of
// each byte reversed, the bytes in place
PPFS_HD inline uint32_t stream_bits(uint32_t le)
{
    le = ((le & 0xF0F0F0F0u) >> 4) | ((le & 0x0F0F0F0Fu) << 4);
    le = ((le & 0xCCCCCCCCu) >> 2) | ((le & 0x33333333u) << 2);
    le = ((le & 0xAAAAAAAAu) >> 1) | ((le & 0x55555555u) << 1);
    return le;
}

// bytes of word w that lie inside a stream of stream_bytes: 4, or fewer for the last word, 0 past it
PPFS_HD inline uint32_t word_bytes(uint64_t w, uint64_t stream_bytes)
{
    const uint64_t at = 4u * w;
    return at >= stream_bytes ? 0u : (stream_bytes - at >= 4u ? 4u : (uint32_t)(stream_bytes - at));
}

// bits i of word w with 32 w + i < nbits
PPFS_HD inline uint32_t tail_mask(uint64_t w, uint64_t nbits)
{
    const uint64_t at = 32u * w;
    return at >= nbits ? 0u : (nbits - at >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(nbits - at)) - 1u);
}

// bits i of word w that bitmap block b covers: stream bits [b * bpb, (b + 1) * bpb), bpb = 8 * ds
PPFS_HD inline uint32_t block_mask(uint64_t w, uint64_t bpb, uint64_t b)
{
    const uint64_t w0 = 32u * w, lo = b * bpb, hi = lo + bpb;
    const uint64_t from = lo > w0 ? lo : w0, to = hi < w0 + 32u ? hi : w0 + 32u;
    if (from >= to)
        return 0u;
    const uint32_t n = (uint32_t)(to - from), sh = (uint32_t)(from - w0);
    return (n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u) << sh;
}

// Src: what the plan reads -- dword(w): the little-endian dword at stream byte 4 w (asked only for a
// word wholly inside the stream), byte(i): stream byte i < stream_bytes, status(b): the decode status
// of bitmap block b < B.

// the bits of every failed bitmap block that word w touches
template <class Src>
PPFS_HD inline uint32_t failed_mask(const Src& src, uint64_t w, uint64_t bpb, uint64_t B)
{
    uint32_t m = 0;
    for (uint64_t b = 32u * w / bpb, last = (32u * w + 31u) / bpb; b <= last && b < B; ++b)
        if (src.status(b) == STATUS_FAILED)
            m |= block_mask(w, bpb, b);
    return m;
}

// word w as the scan sees it: bit i set = image block first_block + 32 w + i is scrubbed
template <class Src>
PPFS_HD inline uint32_t word_bits(const Src& src, uint64_t w, uint64_t nbits, uint64_t ds, uint64_t B)
{
    const uint32_t tail = tail_mask(w, nbits);
    if (!tail)
        return 0u;
    const uint32_t nb = word_bytes(w, B * ds);
    uint32_t le = 0;
    if (nb == 4u) {
        le = src.dword(w);
    } else {
        for (uint32_t k = 0; k < nb; ++k)
            le |= (uint32_t)src.byte(4u * w + k) << (8u * k);
    }
    return (stream_bits(le) | failed_mask(src, w, 8u * ds, B)) & tail;
}

// piece p of the bit range: bits [bit0, bit0 + bits), whose first word is word0 (PIECE_BITS is a
// multiple of 32 and of CHUNK_BITS, so pieces and chunks start on word boundaries)
struct Piece {
    uint64_t bit0, bits, word0;
    uint32_t chunks; // ceil(bits / CHUNK_BITS) <= PIECE_CHUNKS
};
PPFS_HD inline uint64_t pieces_of(uint64_t nbits) { return (nbits + PIECE_BITS - 1u) / PIECE_BITS; }
PPFS_HD inline Piece piece_of(uint64_t nbits, uint64_t p)
{
    const uint64_t bit0 = p * PIECE_BITS, left = nbits - bit0, bits = left < PIECE_BITS ? left : PIECE_BITS;
    return Piece { bit0, bits, bit0 / 32u, (uint32_t)((bits + CHUNK_BITS - 1u) / CHUNK_BITS) };
}

// where a status lands in ppfs_ecc_scrub_counts taken as eight 64-bit words: ok, corrected, failed,
// out_of_range; -1 for a value that is none of the four
PPFS_HD inline int count_slot(uint32_t st) { return st == 0u ? 0 : st == 1u ? 1 : st == 5u ? 2 : st == 9u ? 3 : -1; }
constexpr int SLOT_NOT_ALLOCATED = 4, SLOT_BITMAP = 5; // bitmap_ok, bitmap_corrected, bitmap_failed = 5, 6, 7

} // namespace alloc
} // namespace ppfs
