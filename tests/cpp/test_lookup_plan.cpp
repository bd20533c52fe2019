// test_lookup_plan.cpp -- the rule of the directory lookups (paritypartyfs_amd/csrc/lookup_plan.hpp) on the host,
// against a literal restatement of the reference: _findEntryByName's strlen / strncmp test
// (lib/directory_manager/src/directory_manager.cpp:189-199), _findEntryByInode (:201-210) and the batch loop of
// getInodeByName (:135-163) over _readDirectoryData (:165-187) and a fake readFile that fails at a chosen block.
//
// Names: every entry buffer the reference sees is NUL-terminated and sits in a heap block of exactly its 128 bytes,
// every query string in a heap block of exactly its length + 1, so that a read past either is the sanitizer's to
// report.  Lengths 0, 1, 11, 12, 13, 123; a query that is a proper prefix of the entry and the reverse; garbage behind
// the entry's NUL; a difference in the first, the last and every other byte; duplicates (the first wins); an
// unterminated entry and the queries of 124 bytes and more or without NUL, against the stated rule.
// Failures: ds in {1, 3, 127, 128, 129, 249, 4091} x n in {0, 1, 255, 256, 257, 300, 513} x every (match position or
// none, failing block or none) pair, the plan's decision (last_block, failure_within, answer) against the loop; the
// scan first_failure against failure_within on every pair of the directories of at most 1,024 blocks and on the
// pairs around last(B) of the longer ones.  The cases are counted per outcome and no class may be empty.
// No HIP: built with the host compiler (tests/test_lookup_cpu.py, with the address and undefined-behaviour
// sanitizers).
#include "../../paritypartyfs_amd/csrc/lookup_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace ppfs::lookupplan;

static int g_fail = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail < 20)                                                                                           \
                std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            ++g_fail;                                                                                                  \
        }                                                                                                              \
    } while (0)

// ---- the reference, restated ----
struct DirectoryEntry { // directory.hpp:8-12
    uint32_t inode;
    char name[124];
};
static_assert(sizeof(DirectoryEntry) == 128, "DirectoryEntry");

static bool ref_name_test(const DirectoryEntry& entry, const char* name)
{
    return std::strlen(name) == std::strlen(entry.name) && std::strncmp(entry.name, name, std::strlen(name)) == 0;
}

// ---- the plan's side: words out of exact-size heap blocks ----
static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct HeapEntry { // 128 bytes, exactly
    uint8_t* p;
    HeapEntry(const std::string& name_bytes, uint32_t inode, uint8_t fill)
        : p((uint8_t*)std::malloc(128))
    {
        std::memset(p, fill, 128);
        for (int i = 0; i < 4; ++i)
            p[i] = (uint8_t)(inode >> (8 * i));
        std::memcpy(p + 4, name_bytes.data(), std::min<size_t>(name_bytes.size(), 124));
    }
    HeapEntry(const HeapEntry&) = delete;
    ~HeapEntry() { std::free(p); }
    const DirectoryEntry& ref() const { return *(const DirectoryEntry*)p; }
};
struct HeapQuery { // the 128-byte record, exactly
    uint8_t* p;
    explicit HeapQuery(const std::string& bytes, uint8_t fill = 0)
        : p((uint8_t*)std::malloc(128))
    {
        std::memset(p, fill, 128);
        std::memcpy(p, bytes.data(), std::min<size_t>(bytes.size(), 128));
    }
    HeapQuery(const HeapQuery&) = delete;
    ~HeapQuery() { std::free(p); }
};
static bool plan_name_test(const uint8_t* entry, const uint8_t* query)
{
    const auto qw = [&](uint32_t w) { return le32(query + 4u * w); };
    const auto ew = [&](uint32_t w) { return le32(entry + 4u + 4u * w); };
    const uint32_t L = query_length(qw);
    const bool whole = name_match(ew, qw, L);
    // the kernel's two steps give the same answer
    const bool steps = query_usable(L) && words_agree(ew, qw, 0u, 3u, L + 1u) && words_agree(ew, qw, 3u, NAME_WORDS, L + 1u);
    CHECK(whole == steps);
    return whole;
}

static uint64_t g_name_cases = 0, g_name_matches = 0;
// name: the entry's name (no NUL inside), behind it a NUL and then `fill`; query: a C string.  Both at most 123 bytes
static void name_case(const std::string& name, const std::string& query, uint8_t fill)
{
    std::string stored = name;
    stored.push_back('\0');
    HeapEntry e(stored, 7, fill);
    e.p[127] = 0; // NUL-terminated whatever the fill
    char* c = (char*)std::malloc(query.size() + 1); // exactly the string
    std::memcpy(c, query.c_str(), query.size() + 1);
    HeapQuery q(query, 0);
    const bool ref = ref_name_test(e.ref(), c);
    const bool got = plan_name_test(e.p, q.p);
    CHECK(ref == got);
    CHECK(ref == (name == query));
    // garbage behind the QUERY's NUL is not looked at either
    HeapQuery q2(query + std::string(1, '\0'), 0xC3);
    CHECK(plan_name_test(e.p, q2.p) == ref);
    ++g_name_cases;
    g_name_matches += ref;
    std::free(c);
}

static std::string letters(size_t n, unsigned seed)
{
    std::string s(n, 'a');
    for (size_t i = 0; i < n; ++i)
        s[i] = (char)('a' + (seed * 31u + i * 7u) % 26u);
    return s;
}

static void test_names()
{
    const size_t lengths[] = { 0, 1, 11, 12, 13, 123 };
    const uint8_t fills[] = { 0x00, 0xAA, 0xFF };
    for (uint8_t fill : fills) {
        for (size_t L : lengths) {
            const std::string name = letters(L, (unsigned)L);
            name_case(name, name, fill); // equal
            for (size_t M : lengths) {
                if (M < L)
                    name_case(name, name.substr(0, M), fill); // the query a proper prefix of the entry
                if (M > L)
                    name_case(name, name + letters(M - L, 99), fill); // the entry a proper prefix of the query
                name_case(name, letters(M, 1000u + (unsigned)M), fill); // unrelated
            }
            for (size_t at = 0; at < L; ++at) { // one byte differs: the first, the last, every one between
                std::string other = name;
                other[at] = (char)(other[at] == 'z' ? 'y' : other[at] + 1);
                name_case(name, other, fill);
                name_case(other, name, fill);
            }
            if (L) { // the garbage behind the entry's NUL spells the rest of the query
                HeapEntry e(name.substr(0, L / 2) + std::string(1, '\0') + name.substr(L / 2), 7, fill);
                e.p[127] = 0;
                HeapQuery q(name);
                CHECK(!plan_name_test(e.p, q.p) || L / 2 == L);
                CHECK(ref_name_test(e.ref(), name.c_str()) == plan_name_test(e.p, q.p));
                HeapQuery half(name.substr(0, L / 2));
                CHECK(plan_name_test(e.p, half.p));
            }
        }
    }
    // high bytes compare as bytes
    name_case(std::string("\xC3\xA9t\xC3\xA9"), std::string("\xC3\xA9t\xC3\xA9"), 0xAA);
    name_case(std::string("\xC3\xA9t\xC3\xA9"), std::string("\xC3\xA9t\xC3\xA8"), 0xAA);
    // the stated rule where the reference has none: an unterminated entry matches nothing ...
    {
        const std::string full = letters(124, 5);
        HeapEntry e(full, 9, 0x41);
        for (size_t L : { (size_t)0, (size_t)1, (size_t)12, (size_t)123 }) {
            HeapQuery q(full.substr(0, L));
            CHECK(!plan_name_test(e.p, q.p));
        }
        // ... and so do a query of 124 bytes or more and one without a NUL, even against the same bytes
        HeapQuery q124(full), q127(full + "xyz"), q128(full + "wxyz", 0x42);
        CHECK(query_length([&](uint32_t w) { return le32(q124.p + 4u * w); }) == 124);
        CHECK(query_length([&](uint32_t w) { return le32(q127.p + 4u * w); }) == 127);
        CHECK(query_length([&](uint32_t w) { return le32(q128.p + 4u * w); }) == 128);
        CHECK(!plan_name_test(e.p, q124.p) && !plan_name_test(e.p, q127.p) && !plan_name_test(e.p, q128.p));
        HeapEntry t(full.substr(0, 123) + std::string(1, '\0'), 9, 0x41);
        CHECK(!plan_name_test(t.p, q124.p));
        HeapQuery q123(full.substr(0, 123));
        CHECK(plan_name_test(t.p, q123.p));
    }
    // first_nul over every position of a word pattern
    for (uint32_t at = 0; at <= 128; ++at) {
        uint8_t rec[128];
        std::memset(rec, 0x80, 128); // 0x80 bytes: the zero-byte trick's hard case
        if (at < 128)
            rec[at] = 0;
        CHECK(first_nul([&](uint32_t w) { return le32(rec + 4u * w); }, 128) == at);
        CHECK(first_nul([&](uint32_t w) { return le32(rec + 4u * w); }, 124) == std::min<uint32_t>(at, 124));
        std::memset(rec, 0x01, 128);
        if (at < 128)
            rec[at] = 0;
        if (at + 1 < 128)
            rec[at + 1] = 0;
        CHECK(first_nul([&](uint32_t w) { return le32(rec + 4u * w); }, 128) == at);
    }
    // duplicates resolve to the first; the inode match
    {
        std::vector<HeapEntry*> dir;
        const char* names[] = { "a", "bb", "target", "c", "target", "" };
        for (uint32_t i = 0; i < 6; ++i)
            dir.push_back(new HeapEntry(std::string(names[i]) + std::string(1, '\0'), 100u + i % 3u, 0xEE));
        auto find = [&](const char* s) {
            HeapQuery q(s);
            return first_match(dir.size(), [&](uint64_t e) { return plan_name_test(dir[e]->p, q.p); });
        };
        CHECK(find("target") == 2 && find("") == 5 && find("a") == 0 && find("targe") == NONE && find("target2") == NONE);
        auto by_inode = [&](uint32_t key) { return first_match(dir.size(), [&](uint64_t e) { return inode_match(le32(dir[e]->p), key); }); };
        CHECK(by_inode(100) == 0 && by_inode(101) == 1 && by_inode(102) == 2 && by_inode(103) == NONE);
        CHECK(first_match(0, [](uint64_t) { return true; }) == NONE);
        for (HeapEntry* e : dir)
            delete e;
    }
    CHECK(g_name_cases > 500 && g_name_matches >= 18 && g_name_matches < g_name_cases);
}

// ---- the batch loop over a fake readFile ----
constexpr uint32_t ENTRY_BATCH_SIZE = 256;
struct LoopAnswer {
    uint32_t status, entry;
};
// n entries of a directory, the first matching entry at `match` (NONE: none), file block `bad` fails with bad_status
// (NO_FAILURE: none).  readFile(offset, size) touches the file blocks offset / ds .. (offset + size - 1) / ds and
// fails as a whole when `bad` is among them
static LoopAnswer reference_loop(uint64_t n, uint64_t ds, uint32_t match, uint64_t bad, uint32_t bad_status)
{
    uint64_t checked = 0;
    while (checked < n) {
        const uint64_t size = std::min<uint64_t>(ENTRY_BATCH_SIZE, n - checked);
        const uint64_t offset = checked * 128u, bytes = size * 128u;
        const uint64_t first = offset / ds, last = (offset + bytes - 1u) / ds;
        if (bad != NO_FAILURE && first <= bad && bad <= last)
            return LoopAnswer { bad_status, NONE };
        if (match != NONE && match >= checked && match < checked + size) // _findEntryBy...: the first match of the batch
            return LoopAnswer { ST_OK, match };
        checked += size;
    }
    return LoopAnswer { ST_NOT_FOUND, NONE };
}

// outcomes: a failing block in front of the match's block or under it (failed before), behind the match in its batch
// (failed behind), anywhere up to the end without a match (failed, no match), behind last(B) (ignored)
static uint64_t g_found = 0, g_not_found = 0, g_failed_before = 0, g_failed_behind = 0, g_failed_no_match = 0, g_ignored = 0;

static void pair(uint64_t n, uint64_t ds, uint32_t match, uint64_t bad, bool scan)
{
    const uint32_t bad_status = (bad % 3u) ? ST_FAILED : ST_OUT;
    const LoopAnswer ref = reference_loop(n, ds, match, bad, bad_status);
    uint32_t failure = 0;
    if (n) {
        const uint64_t last = last_block(n, match, ds);
        failure = failure_within(last, bad, bad_status);
        if (scan)
            CHECK(failure == first_failure(last, [&](uint64_t j) { return j == bad ? bad_status : (j % 2u ? 1u : 0u); }));
    }
    const Hit h = answer(n, match, failure, match == NONE ? NONE : 5000u + match);
    CHECK(h.status == ref.status && h.entry == ref.entry && h.reserved == 0);
    CHECK(h.inode == (h.status == ST_OK ? 5000u + match : NONE));
    CHECK(count_slot(h.status) == (h.status == ST_OK ? 0 : h.status == ST_NOT_FOUND ? 1 : h.status == ST_FAILED ? 2 : 3));
    if (h.status == ST_FAILED || h.status == ST_OUT) {
        if (match == NONE)
            ++g_failed_no_match;
        else if (bad <= ((uint64_t)match * 128u + 127u) / ds)
            ++g_failed_before;
        else
            ++g_failed_behind; // under later entries of the match's batch: the loop's readFile fails as a whole
    }
    else if (bad != NO_FAILURE)
        ++g_ignored; // a failing block behind last(B)
    else if (h.status == ST_OK)
        ++g_found;
    else
        ++g_not_found;
}

static void test_failures()
{
    const uint64_t sizes[] = { 1, 3, 127, 128, 129, 249, 4091 };
    const uint64_t counts[] = { 0, 1, 255, 256, 257, 300, 513 };
    for (uint64_t ds : sizes)
        for (uint64_t n : counts) {
            const uint64_t blocks = (n * 128u + ds - 1u) / ds;
            CHECK(entries_of(n * 128u + 127u) == n && chunks_of(n) == (n + 255u) / 256u);
            for (uint64_t mi = 0; mi <= n; ++mi) {
                const uint32_t match = mi == n ? NONE : (uint32_t)mi;
                pair(n, ds, match, NO_FAILURE, true);
                const uint64_t last = n ? last_block(n, match, ds) : 0;
                for (uint64_t bad = 0; bad < blocks; ++bad)
                    pair(n, ds, match, bad, blocks <= 1024u || (bad + 2u >= last && bad <= last + 2u));
            }
        }
    // the cases the issue names, at ds = 249
    CHECK(reference_loop(300, 249, 10, 200u * 128u / 249u, ST_FAILED).status == ST_FAILED); // behind the match, same batch
    CHECK(failure_within(last_block(300, 10, 249), 200u * 128u / 249u, ST_FAILED) == ST_FAILED);
    const uint64_t straddler = 32768u / 249u; // holds bytes 32,619 .. 32,867: the end of batch 0 and the start of batch 1
    CHECK(straddler * 249u < 32768u && (straddler + 1u) * 249u > 32768u);
    CHECK(reference_loop(300, 249, 10, straddler, ST_FAILED).status == ST_FAILED && last_block(300, 10, 249) == straddler);
    CHECK(reference_loop(300, 249, 260, straddler, ST_FAILED).status == ST_FAILED && last_block(300, 260, 249) > straddler);
    CHECK(reference_loop(300, 249, 10, straddler + 1u, ST_FAILED).status == ST_OK); // behind last(0): ignored
    CHECK(answer(0, NONE, ST_FAILED, 1).status == ST_NOT_FOUND); // an empty directory reads nothing
    CHECK(g_found > 0 && g_not_found > 0 && g_failed_before > 0 && g_failed_behind > 0 && g_failed_no_match > 0 && g_ignored > 0);
}

int main()
{
    test_names();
    test_failures();
    std::printf("names: %llu cases, %llu matches; pairs: %llu found, %llu not found, %llu failed before, %llu failed behind, "
                "%llu failed without a match, %llu failing behind last(B) and ignored\n",
        (unsigned long long)g_name_cases, (unsigned long long)g_name_matches, (unsigned long long)g_found,
        (unsigned long long)g_not_found, (unsigned long long)g_failed_before, (unsigned long long)g_failed_behind,
        (unsigned long long)g_failed_no_match, (unsigned long long)g_ignored);
    if (g_fail) {
        std::printf("%d CHECKS FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
