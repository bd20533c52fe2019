// test_files_plan.cpp -- csrc/files_plan.hpp (the arithmetic of the walk over a batch of files) against brute
// force: a per-file loop of the single-file plan of csrc/file_plan.hpp.  A plain host program: built with
// g++ -fsanitize=address,undefined by tests/test_files_cpu.py; the merged expansion runs over heap buffers of
// exactly the merged scratch's size, so a read past its end is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../paritypartyfs_amd/csrc/file_plan.hpp"
#include "../../paritypartyfs_amd/csrc/files_plan.hpp"

using namespace ppfs::fileplan;
namespace fp = ppfs::filesplan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (++g_fail <= 20) {                                                                                      \
                std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond);                                             \
                std::printf(__VA_ARGS__);                                                                              \
                std::printf("\n");                                                                                     \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static uint32_t g_seed = 2024;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }
static uint64_t rnd_below(uint64_t n) { return n ? (((uint64_t)rnd() << 16) ^ rnd()) % n : 0; }

struct File {
    uint32_t rec[16];
    uint64_t offset, nbytes;   // its range
    uint64_t first, count;     // the blocks the range must touch
    uint64_t bytes;            // the bytes it must deliver
};

// a file whose range touches the file blocks [first, first + count): starts and ends in mid-block, now and
// then asks for more than the file holds; count == 0: an empty range
static File make_file(uint64_t ds, uint64_t first, uint64_t count)
{
    File f {};
    for (int d = 0; d < 15; ++d)
        f.rec[d] = rnd();
    f.first = count ? first : 0;
    f.count = count;
    if (count == 0) {
        f.offset = rnd_below(1000);
        f.nbytes = 0;
        f.rec[15] = rnd() % 3 ? (uint32_t)rnd_below(5000) : 0u;
        return f;
    }
    const uint64_t o0 = rnd_below(ds), lo = (count - 1) * ds > o0 ? (count - 1) * ds - o0 + 1 : 1, hi = count * ds - o0;
    f.offset = first * ds + o0;
    f.bytes = lo + rnd_below(hi - lo + 1);
    const bool clamp = rnd() % 4 == 0;
    f.nbytes = clamp ? f.bytes + 1 + rnd_below(1000) : f.bytes;
    f.rec[15] = (uint32_t)(f.offset + f.bytes + (clamp ? 0 : rnd_below(3 * ds)));
    return f;
}

// the scratch of an expansion, single-file or merged
struct Mem {
    const uint8_t *payload, *st, *inh;
    uint32_t status(uint64_t p) const { return st[p]; }
    uint32_t inherited(uint64_t p) const { return inh[p]; }
    uint32_t payload_byte(uint64_t at) const { return payload[at]; }
};
struct Src : Mem {
    const uint32_t* file;
    uint32_t inode(uint32_t dw) const { return file[dw]; }
};

static void check_batch(uint64_t ds, const std::vector<File>& files, bool whole)
{
    const uint64_t I = ipb_of(ds), n = files.size();
    std::vector<uint32_t> recs(16 * n);
    std::vector<uint64_t> ranges(2 * n);
    for (uint64_t f = 0; f < n; ++f) {
        for (int d = 0; d < 16; ++d)
            recs[16 * f + d] = files[f].rec[d];
        ranges[2 * f] = files[f].offset;
        ranges[2 * f + 1] = files[f].nbytes;
    }
    fp::Plan plan;
    uint64_t bad = 99;
    const int r = fp::build(recs.data(), whole ? nullptr : ranges.data(), n, ds, plan, &bad);
    CHECK(r == fp::RANGE_OK, "ds %llu: a valid batch is refused (%d, file %llu)", (unsigned long long)ds, r, (unsigned long long)bad);
    if (r != fp::RANGE_OK)
        return;

    // ---- slots and totals: the single-file plan, file by file ----
    std::vector<Tree> trees(n);
    uint64_t tot_blocks = 0, tot_bytes = 0, tot[3] = { 0, 0, 0 };
    for (uint64_t f = 0; f < n; ++f) {
        const Span sp = whole ? span(files[f].rec[15], ds, 0, files[f].rec[15]) : span(files[f].rec[15], ds, files[f].offset, files[f].nbytes);
        CHECK(sp.ok, "the test's own range");
        if (!whole)
            CHECK(sp.first == files[f].first && sp.count == files[f].count && sp.bytes == files[f].bytes, "the test's own range");
        trees[f] = tree_of(sp.first, sp.count, I);
        const fp::Slot& s = plan.slots[f];
        CHECK(s.first == sp.first && s.blocks == sp.count && s.bytes == sp.bytes, "file %llu span", (unsigned long long)f);
        CHECK(s.block_pos == tot_blocks && s.out_pos == tot_bytes, "file %llu positions", (unsigned long long)f);
        for (int l = 0; l < 3; ++l)
            CHECK(s.tree_n[l] == level_count(trees[f], l), "file %llu level %d count", (unsigned long long)f, l);
        tot_blocks += sp.count;
        tot_bytes += sp.bytes;
        for (int l = 0; l < 3; ++l)
            tot[l] += level_count(trees[f], l);
    }
    CHECK(plan.total.blocks == tot_blocks && plan.total.bytes == tot_bytes, "totals");
    CHECK(plan.total.tree[0] == tot[0] && plan.total.tree[1] == tot[1] && plan.total.tree[2] == tot[2]
            && plan.total.tree_blocks == tot[0] + tot[1] + tot[2],
        "tree totals");
    const uint64_t ebase[3] = { 0, tot[0], tot[0] + tot[1] };
    const uint64_t sbase[3] = { 0, round16(tot[0]), round16(tot[0]) + round16(tot[1]) };
    CHECK(plan.levels.base[0] == sbase[0] && plan.levels.base[1] == sbase[1] && plan.levels.base[2] == sbase[2], "scratch bases");
    CHECK(plan.levels.slots == (tot[0] + tot[1] + tot[2] ? sbase[2] + tot[2] : 0), "scratch slots");
    uint64_t run[3] = { 0, 0, 0 };
    for (uint64_t f = 0; f < n; ++f) { // level-major: level l of file f follows level l of the files before it
        for (int l = 0; l < 3; ++l) {
            CHECK(plan.slots[f].tree_pos[l] == ebase[l] + run[l], "file %llu level %d position", (unsigned long long)f, l);
            CHECK(plan.recs[f].lvl[l] == sbase[l] + run[l], "file %llu level %d scratch position", (unsigned long long)f, l);
            run[l] += level_count(trees[f], l);
        }
        const fp::FileRec& q = plan.recs[f];
        CHECK(q.first == plan.slots[f].first && q.blocks == plan.slots[f].blocks && q.bytes == plan.slots[f].bytes
                && q.out_pos == plan.slots[f].out_pos,
            "file %llu record", (unsigned long long)f);
        CHECK(q.off0 == (whole || !q.blocks ? 0 : files[f].offset % ds), "file %llu off0", (unsigned long long)f);
        for (int d = 0; d < 16; ++d)
            CHECK(q.inode[d] == files[f].rec[d], "file %llu inode", (unsigned long long)f);
    }

    // ---- row tables: every entry's owner by brute force, row_of, the span of 256 entries ----
    for (int l = 0; l < fp::LEVELS; ++l) {
        std::vector<std::pair<uint64_t, uint64_t>> owner; // (file, k) of every merged entry
        uint64_t nonempty = 0;
        for (uint64_t f = 0; f < n; ++f) {
            const uint64_t c = level_count(trees[f], l);
            nonempty += c > 0;
            for (uint64_t k = 0; k < c; ++k)
                owner.push_back({ f, k });
        }
        const std::vector<fp::Row>& rows = plan.rows[l];
        CHECK(rows.size() == nonempty + 1, "level %d rows", l);
        if (rows.size() != nonempty + 1)
            continue;
        CHECK(rows.back().first == owner.size() && rows.back().file == n, "level %d sentinel", l);
        for (uint64_t q = 0; q + 1 < rows.size(); ++q)
            CHECK(rows[q].first < rows[q + 1].first && rows[q].file < n && (q == 0 || rows[q - 1].file < rows[q].file),
                "level %d row %llu", l, (unsigned long long)q);
        // the table as the device sees it: a heap copy WITHOUT the sentinel, so that row_of reading it is a report
        std::vector<fp::Row> bare(rows.begin(), rows.end() - 1);
        for (uint64_t e = 0; e < owner.size(); ++e) {
            const uint64_t q = fp::row_of(bare.data(), bare.size(), e);
            CHECK(q < bare.size() && bare[q].file == owner[e].first && e - bare[q].first == owner[e].second, "level %d entry %llu owner",
                l, (unsigned long long)e);
        }
        for (uint64_t w = 0; w < owner.size(); w += 64) {
            const uint64_t last = w + 255 < owner.size() ? w + 255 : owner.size() - 1;
            CHECK(fp::row_of(bare.data(), bare.size(), last) - fp::row_of(bare.data(), bare.size(), w) + 1 <= 256, "level %d window", l);
        }
    }

    // ---- the merged expansion against the single-file one, level by level, with statuses 1 / 5 / 9 ----
    const uint64_t slots = plan.levels.slots;
    std::vector<uint8_t> mpay(slots * ds, 0xEE), mst(slots, 0xEE), minh(slots, 0xEE);
    const Mem mem { mpay.data(), mst.data(), minh.data() };
    std::vector<std::vector<uint8_t>> spay(n), sst(n), sinh(n);
    for (uint64_t f = 0; f < n; ++f) {
        const uint64_t s1 = tree_blocks(trees[f]) ? tree_slots(trees[f]) : 0;
        spay[f].assign(s1 * ds, 0xEE);
        sst[f].assign(s1, 0);
        sinh[f].assign(s1, 0);
    }
    for (int l = 0; l <= LEVEL_DATA; ++l)
        for (uint64_t f = 0; f < n; ++f) {
            Src src;
            src.payload = spay[f].data();
            src.st = sst[f].data();
            src.inh = sinh[f].data();
            src.file = files[f].rec;
            const Tree& t = trees[f];
            for (uint64_t k = 0, c = level_count(t, l); k < c; ++k) {
                const Expanded a = expand(t, l, k, ds, src), b = fp::expand_entry(plan.recs[f], l, k, ds, mem);
                CHECK(a.pointer == b.pointer && a.inherited == b.inherited, "ds %llu file %llu level %d entry %llu: %u/%u vs %u/%u",
                    (unsigned long long)ds, (unsigned long long)f, l, (unsigned long long)k, a.pointer, a.inherited, b.pointer, b.inherited);
                if (l == LEVEL_DATA)
                    continue;
                // what the list decode leaves for this entry, in both scratches
                const uint32_t pick = rnd() % 8;
                const uint8_t st = a.inherited ? 9 : pick == 0 ? 5 : pick == 1 ? 9 : pick == 2 ? 1 : 0;
                const uint64_t one = slot_base(t, l) + k, many = plan.recs[f].lvl[l] + k;
                sst[f][one] = mst[many] = st;
                sinh[f][one] = minh[many] = a.inherited;
                if (st == 5 || st == 9)
                    continue; // payload undefined
                for (uint64_t q = 0; q < ds; ++q)
                    spay[f][one * ds + q] = mpay[many * ds + q] = (uint8_t)rnd();
            }
            const Expanded past = fp::expand_entry(plan.recs[f], l, level_count(t, l), ds, mem);
            CHECK(past.pointer == NO_BLOCK && past.inherited == STATUS_OUT, "an entry past its file's level names no block");
        }
}

// every (first, count) shape of the small trees; the large trees' edges, and 40 drawn
static std::vector<std::pair<uint64_t, uint64_t>> shapes_of(uint64_t ds)
{
    const uint64_t I = ipb_of(ds), cap = capacity_ipb(I);
    std::vector<std::pair<uint64_t, uint64_t>> shapes;
    if (I <= 3) {
        for (uint64_t first = 0; first < cap; ++first)
            for (uint64_t count = 0; first + count <= cap; ++count)
                shapes.push_back({ first, count });
        return shapes;
    }
    const uint64_t edges[] = { 0, 1, 11, 12, 13, 12 + I - 1, 12 + I, 12 + I + 1, 12 + I + I * I - 1, 12 + I + I * I, 12 + I + I * I + I,
        cap - 1 };
    for (uint64_t a : edges)
        for (uint64_t b : edges)
            if (a <= b)
                shapes.push_back({ a, b - a + (b < cap ? 1 : 0) });
    for (int q = 0; q < 40; ++q) {
        const uint64_t first = rnd_below(cap);
        shapes.push_back({ first, rnd_below(cap - first + 1) });
    }
    return shapes;
}

// build_one, the plan of the single-file calls (which know their range as blocks), against build() of a batch of
// that one file and the equivalent byte range: the same slot, record, rows, totals and levels; and the scratch
// layout is the single-file one of file_plan.hpp
static void test_one_file()
{
    for (uint64_t ds : { (uint64_t)2, (uint64_t)3, (uint64_t)5, (uint64_t)9, (uint64_t)12, (uint64_t)16, (uint64_t)58, (uint64_t)508 })
        for (const std::pair<uint64_t, uint64_t>& sh : shapes_of(ds)) {
            const File f = make_file(ds, sh.first, sh.second);
            const uint64_t range[2] = { f.offset, f.nbytes };
            fp::Plan batch;
            fp::OnePlan one;
            uint64_t bad = 99;
            const int r = fp::build(f.rec, range, 1, ds, batch, &bad);
            CHECK(r == fp::RANGE_OK, "ds %llu: a valid file is refused (%d)", (unsigned long long)ds, r);
            if (r != fp::RANGE_OK)
                continue;
            const Span sp = span(f.rec[15], ds, f.offset, f.nbytes);
            CHECK(sp.ok && sp.first == f.first && sp.count == f.count && sp.bytes == f.bytes, "the test's own range");
            fp::build_one(f.rec, sp.first, sp.count, f.offset % ds, sp.bytes, ds, one);
            const unsigned long long a = sp.first, b = sp.count;
            CHECK(!std::memcmp(&one.slot, &batch.slots[0], sizeof(fp::Slot)), "ds %llu [%llu, +%llu): slot", (unsigned long long)ds, a, b);
            CHECK(!std::memcmp(&one.one.rec, &batch.recs[0], sizeof(fp::FileRec)), "ds %llu [%llu, +%llu): record", (unsigned long long)ds, a, b);
            CHECK(!std::memcmp(&one.total, &batch.total, sizeof(fp::Totals)), "ds %llu [%llu, +%llu): totals", (unsigned long long)ds, a, b);
            CHECK(!std::memcmp(&one.levels, &batch.levels, sizeof(fp::Levels)), "ds %llu [%llu, +%llu): levels", (unsigned long long)ds, a, b);
            // the two views: what the walk reads
            const fp::PlanView v1 = one.view(), vb = batch.view();
            CHECK(v1.nfiles == 1 && vb.nfiles == 1 && v1.recs == &one.one.rec && !std::memcmp(&v1.total, &vb.total, sizeof(fp::Totals))
                    && !std::memcmp(&v1.levels, &vb.levels, sizeof(fp::Levels)),
                "ds %llu [%llu, +%llu): views", (unsigned long long)ds, a, b);
            for (int l = 0; l < fp::LEVELS; ++l) {
                CHECK(v1.nrows[l] == vb.nrows[l] && vb.nrows[l] + 1 == batch.rows[l].size(), "ds %llu [%llu, +%llu): level %d rows",
                    (unsigned long long)ds, a, b, l);
                for (size_t q = 0; q <= v1.nrows[l] && q <= vb.nrows[l]; ++q) // the sentinel too
                    CHECK(v1.rows[l][q].first == vb.rows[l][q].first && v1.rows[l][q].file == vb.rows[l][q].file
                            && v1.rows[l][q].pad == vb.rows[l][q].pad,
                        "ds %llu [%llu, +%llu): level %d row %llu", (unsigned long long)ds, a, b, l, (unsigned long long)q);
            }
            const Tree t = tree_of(sp.first, sp.count, ipb_of(ds));
            const Tree& u = one.one.tree;
            CHECK(u.j0 == t.j0 && u.j1 == t.j1 && u.I == t.I && u.S1 == t.S1 && u.S2 == t.S2 && u.a_ind == t.a_ind && u.a_dbl == t.a_dbl
                    && u.a_trb == t.a_trb && u.d0 == t.d0 && u.d1 == t.d1 && u.t0 == t.t0 && u.t1 == t.t1 && u.nA == t.nA && u.nBd == t.nBd
                    && u.nBt == t.nBt && u.nB == t.nB && u.nC == t.nC,
                "ds %llu [%llu, +%llu): the range's tree", (unsigned long long)ds, a, b);
            if (tree_blocks(t)) {
                for (int l = 0; l < 3; ++l)
                    CHECK(one.one.rec.lvl[l] == slot_base(t, l), "ds %llu [%llu, +%llu): level %d starts at the single-file slot",
                        (unsigned long long)ds, a, b, l);
                CHECK(one.levels.slots == tree_slots(t), "ds %llu [%llu, +%llu): the single-file scratch slots", (unsigned long long)ds, a, b);
            } else {
                CHECK(one.levels.slots == 0, "ds %llu [%llu, +%llu): no tree, no slots", (unsigned long long)ds, a, b);
            }
        }
}

static void test_batches()
{
    for (uint64_t ds : { (uint64_t)3, (uint64_t)5, (uint64_t)9, (uint64_t)12, (uint64_t)58 }) {
        const uint64_t I = ipb_of(ds), cap = capacity_ipb(I);
        const std::vector<std::pair<uint64_t, uint64_t>> shapes = shapes_of(ds);
        for (size_t s = 0; s < shapes.size(); ++s) {
            const uint64_t nfiles = 1 + s % 6;
            std::vector<File> files;
            for (uint64_t f = 0; f < nfiles; ++f) {
                const uint32_t kind = rnd() % 5;
                std::pair<uint64_t, uint64_t> sh = f == s % nfiles ? shapes[s] : shapes[rnd_below(shapes.size())];
                if (f != s % nfiles && kind == 0)
                    sh.second = 0; // empty files, often several in a row
                if (f != s % nfiles && kind == 1 && !files.empty() && files.back().count == 0)
                    sh.second = 0;
                files.push_back(make_file(ds, sh.first, sh.second));
            }
            check_batch(ds, files, false);
        }
        // every file whole (ranges == NULL), empty files among them
        for (int q = 0; q < 30; ++q) {
            std::vector<File> files;
            for (uint64_t f = 0, nfiles = 1 + rnd() % 6; f < nfiles; ++f) {
                File x = make_file(ds, 0, rnd() % 3 ? rnd_below(cap < 300 ? cap + 1 : 300) : 0);
                if (x.count == 0)
                    x.rec[15] = 0;
                else
                    x.rec[15] = (uint32_t)((x.count - 1) * ds + 1 + rnd_below(ds));
                files.push_back(x);
            }
            check_batch(ds, files, true);
        }
        // all empty, and a batch of none
        check_batch(ds, { make_file(ds, 0, 0), make_file(ds, 0, 0), make_file(ds, 0, 0) }, false);
        check_batch(ds, {}, false);
    }
    // many small files: a window of 256 entries spans 256 rows, runs of empty files in between
    std::vector<File> many;
    for (int f = 0; f < 700; ++f)
        many.push_back(make_file(58, 0, f % 50 < 5 ? 0 : f % 7 == 0 ? 2 : 1));
    many.push_back(make_file(58, 3, 400));
    for (int f = 0; f < 300; ++f)
        many.push_back(make_file(58, 20, f % 3 ? 1 : 8));
    check_batch(58, many, false);
}

static void test_refusals()
{
    const uint64_t ds = 12, cap = capacity(ds);
    std::vector<File> files = { make_file(ds, 0, 3), make_file(ds, 2, 5), make_file(ds, 0, 0) };
    auto run = [&](uint64_t* bad) {
        std::vector<uint32_t> recs;
        std::vector<uint64_t> ranges;
        for (const File& f : files) {
            recs.insert(recs.end(), f.rec, f.rec + 16);
            ranges.push_back(f.offset);
            ranges.push_back(f.nbytes);
        }
        fp::Plan plan;
        return fp::build(recs.data(), ranges.data(), files.size(), ds, plan, bad);
    };
    uint64_t bad = 99;
    CHECK(run(&bad) == fp::RANGE_OK, "a valid batch");
    files[1].offset = files[1].rec[15]; // at the end, nbytes > 0
    CHECK(run(&bad) == fp::BAD_OFFSET && bad == 1, "offset at the file's end: file %llu", (unsigned long long)bad);
    files[1].nbytes = 0; // ... is a valid empty range
    CHECK(run(&bad) == fp::RANGE_OK, "nbytes == 0 anywhere");
    files[2].rec[15] = 0xFFFFFFFFu;
    files[2].offset = (cap - 1) * ds;
    files[2].nbytes = ds;
    CHECK(run(&bad) == fp::RANGE_OK, "the last block of the tree");
    files[2].nbytes = ds + 1;
    CHECK(run(&bad) == fp::BAD_CAPACITY && bad == 2, "past the capacity: file %llu", (unsigned long long)bad);
}

int main()
{
    test_batches();
    test_one_file();
    test_refusals();
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
