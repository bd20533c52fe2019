#pragma once
// lookup_plan.hpp -- the rule of the directory lookups (lookup_path.cpp, dir_walk.hip; include/ppfs_ecc.h
// ppfs_ecc_lookup_*): what DirectoryManager::getInodeByName (lib/directory_manager/src/directory_manager.cpp:135-163)
// and the search inside removeEntry (:67-90) answer for one (directory, key), as plain arithmetic.  For host and
// device alike, so the kernels, the host form and tests/cpp/test_lookup_plan.cpp (the same rule against a literal
// strlen / strncmp restatement and a literal batch loop, under the sanitizers) decide identically.
//
// Entries.  A directory of file_size bytes has n = file_size / 128 entries; trailing bytes are never read.  Entry e is
// the 128 bytes at 128 e of the payload (DirectoryEntry, directory.hpp:8-12): bytes [0, 4) the little-endian inode
// number, bytes [4, 128) the 124 name bytes.  Taken as 32 little-endian words, word 0 is the inode number and word
// 1 + j is name word j.  A query's key is a 128-byte record whose name starts at byte 0: its word j goes with the
// entry's name word j.
// Name match (_findEntryByName, :189-199).  The entry's name length is the position of the first NUL in its 124 name
// bytes; a query of length L matches when that length is L and the L bytes are equal, which is: the entry's name
// bytes [0, L] equal the query's bytes [0, L], the NUL included.  Bytes behind the entry's NUL are not looked at.  L
// is the position of the first NUL of the query's 128 bytes; a query with L >= 124 or no NUL matches nothing.
// DEVIATION: an entry with no NUL in its 124 name bytes matches nothing.  The reference's strlen would run on into
// the next entry's inode number and name.
// Inode match (_findEntryByInode, :201-210).  Entry word 0 equals the key.
// First match.  m is the lowest matching entry below n; NONE when there is none.
// The loop's failure rule.  The reference reads batch b, entries [256 b, min(256 b + 256, n)), with one readFile, and
// the whole batch fails if any file block under those bytes fails, blocks under entries behind a match included.
// With B = m / 256 for a match and the last batch otherwise, last(B) is the last file block batch B's bytes touch.
// The lowest file block j <= last(B) whose final read status is 5 or 9 gives the query that status and no inode;
// without one the answer is (0, inode, m) or NOT_FOUND.  A failing block behind last(B) does not matter.  n == 0 is
// NOT_FOUND with nothing read.
#include <stdint.h>

#if defined(__HIPCC__)
#define PPFS_HD __host__ __device__
#else
#define PPFS_HD
#endif

namespace ppfs {
namespace lookupplan {

constexpr uint32_t ENTRY_BYTES = 128, NAME_BYTES = 124, NAME_WORDS = 31, QUERY_BYTES = 128, QUERY_WORDS = 32;
constexpr uint32_t BATCH = 256;        // ENTRY_BATCH_SIZE: entries per readFile of the loop
constexpr uint32_t NONE = 0xFFFFFFFFu; // no match; also the inode and entry of a hit whose status is not 0
constexpr uint32_t ST_OK = 0, ST_NOT_FOUND = 2, ST_FAILED = 5, ST_OUT = 9; // ST_NOT_FOUND: PPFS_ECC_NOT_FOUND
constexpr int MODE_NAME = 0, MODE_INODE = 1;

PPFS_HD inline uint64_t entries_of(uint64_t file_size) { return file_size / ENTRY_BYTES; }

// The position of the first NUL among the first nbytes bytes of the little-endian words word(0), word(1), ...;
// nbytes when there is none.
template <class Word>
PPFS_HD inline uint32_t first_nul(Word word, uint32_t nbytes)
{
    for (uint32_t w = 0; 4u * w < nbytes; ++w) {
        const uint32_t x = word(w), z = (x - 0x01010101u) & ~x & 0x80808080u; // its lowest set bit marks the first zero byte
        if (z) {
            const uint32_t at = 4u * w + ((uint32_t)__builtin_ctz(z) >> 3);
            return at < nbytes ? at : nbytes;
        }
    }
    return nbytes;
}
// L of a query record; a query whose L is not below NAME_BYTES matches nothing
template <class Word>
PPFS_HD inline uint32_t query_length(Word query_word) { return first_nul(query_word, QUERY_BYTES); }
PPFS_HD inline bool query_usable(uint32_t L) { return L < NAME_BYTES; }

// Do name words [w0, w1) of an entry and of a query agree on the name bytes below `need`?  need = L + 1 compares the
// query's NUL as well, so a whole-name match is words_agree(.., 0, NAME_WORDS, L + 1) for a usable L: words at or
// past `need` are not looked at.  The kernel asks in two steps, words [0, 3) out of the entry's first 16 bytes, then
// the rest.
template <class EntryName, class Query>
PPFS_HD inline bool words_agree(EntryName entry_name_word, Query query_word, uint32_t w0, uint32_t w1, uint32_t need)
{
    for (uint32_t w = w0; w < w1 && 4u * w < need; ++w) {
        const uint32_t left = need - 4u * w, mask = left >= 4u ? 0xFFFFFFFFu : (1u << (8u * left)) - 1u;
        if ((entry_name_word(w) ^ query_word(w)) & mask)
            return false;
    }
    return true;
}
template <class EntryName, class Query>
PPFS_HD inline bool name_match(EntryName entry_name_word, Query query_word, uint32_t L)
{
    return query_usable(L) && words_agree(entry_name_word, query_word, 0u, NAME_WORDS, L + 1u);
}
PPFS_HD inline bool inode_match(uint32_t entry_word0, uint32_t key) { return entry_word0 == key; }

// last(B): n > 0 entries, m the first match or NONE, ds > 0
PPFS_HD inline uint64_t last_block(uint64_t n, uint32_t m, uint64_t ds)
{
    const uint64_t B = m != NONE ? m / BATCH : (n - 1u) / BATCH;
    const uint64_t end = (B + 1u) * BATCH < n ? (B + 1u) * BATCH : n;
    return (end * ENTRY_BYTES - 1u) / ds;
}
PPFS_HD inline bool fails(uint32_t status) { return status == ST_FAILED || status == ST_OUT; }
// the status of the lowest failing file block j <= last, 0 when none fails (the host's scan; the finish kernel runs
// the same predicate a wave at a time)
template <class Status>
PPFS_HD inline uint32_t first_failure(uint64_t last, Status status)
{
    for (uint64_t j = 0; j <= last; ++j) {
        const uint32_t s = status(j);
        if (fails(s))
            return s;
    }
    return 0u;
}

// The same decision from a directory's lowest failing file block, found once for all its queries (the host form):
// lowest = NO_FAILURE when no block of the directory fails
constexpr uint64_t NO_FAILURE = ~0ull;
PPFS_HD inline uint32_t failure_within(uint64_t last, uint64_t lowest, uint32_t lowest_status) { return lowest <= last ? lowest_status : 0u; }

// m: the lowest entry below n for which match(e) holds, NONE when there is none (the host's search; the match kernel
// takes the minimum over its waves)
template <class Match>
PPFS_HD inline uint32_t first_match(uint64_t n, Match match)
{
    for (uint64_t e = 0; e < n && e < NONE; ++e)
        if (match(e))
            return (uint32_t)e;
    return NONE;
}

// the hit record of a query: ppfs_ecc_lookup_hit
struct Hit {
    uint32_t inode, entry, status, reserved;
};
// n: the directory's entries; m: the first match or NONE; failure: first_failure over [0, last_block(n, m, ds)], not
// looked at for n == 0; inode: entry m's word 0, not looked at unless the answer is a hit
PPFS_HD inline Hit answer(uint64_t n, uint32_t m, uint32_t failure, uint32_t inode)
{
    if (n == 0)
        return Hit { NONE, NONE, ST_NOT_FOUND, 0u };
    if (failure)
        return Hit { NONE, NONE, failure, 0u };
    if (m == NONE)
        return Hit { NONE, NONE, ST_NOT_FOUND, 0u };
    return Hit { inode, m, ST_OK, 0u };
}

// where a query's status lands in ppfs_ecc_lookup_counts taken as eight 64-bit words: found, not_found, failed,
// out_of_range; -1 for any other value
PPFS_HD inline int count_slot(uint32_t st) { return st == ST_OK ? 0 : st == ST_NOT_FOUND ? 1 : st == ST_FAILED ? 2 : st == ST_OUT ? 3 : -1; }

// what the kernels need of one directory (32 bytes), and a query as it travels (ppfs_ecc_lookup_query)
struct DirRec {
    uint64_t n;         // entries
    uint64_t out_pos;   // where its entries start in the entries buffer
    uint64_t block_pos; // where its file blocks start in the block status array
    uint64_t blocks;    // its file blocks
};
struct Query {
    uint32_t dir, key;
};
static_assert(sizeof(DirRec) == 32 && sizeof(Query) == 8 && sizeof(Hit) == 16, "table records");

// the match kernel's walk: a wave takes CHUNK entries at a time, one per lane and step
constexpr uint32_t CHUNK = 256;
PPFS_HD inline uint64_t chunks_of(uint64_t n) { return (n + CHUNK - 1u) / CHUNK; }

} // namespace lookupplan
} // namespace ppfs
