// test_block_file.cpp -- fileBlocks / readFile of the C++ adapter (include/ppfs_gpu/block_device.hpp) on the
// GPU, differentially: each call on one device is compared with the default per-block loop (the read-only
// BlockIndexIterator walk through readBlock, IBlockDevice::fileBlocks / readFile) on a second device over a
// copy of the disk -- result, blocks or bytes, the whole disk image and the correction log in order.  Where a
// block fails, the comparison covers the result and everything up to that block: the engine calls attempt
// every block, so later ones may additionally have been corrected and logged.
// The file is written through the adapter the way the reference writes one: index blocks by a write of
// their entries at {block, 0}, data blocks whole, all placed by a seeded permutation.
// Disks: StackDisk and MappedFileDisk (mapped: engine calls on the image) and a plain in-memory disk
// without a mapping (the per-block loop).
//
// usage: test_block_file <directory for the file-backed disks>
// Exit status 0 and "ALL PASSED" on success.  Needs a GPU (the adapter has no CPU fallback).
#include "ppfs_gpu/block_device.hpp"

#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <vector>

using namespace ppfs_gpu;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define EXPECT_TRUE(c)                                                                                   \
    do {                                                                                                 \
        ++g_checks;                                                                                      \
        if (!(c)) {                                                                                      \
            if (++g_fail < 40)                                                                           \
                std::fprintf(stderr, "FAIL %s:%d [%s]: %s\n", __FILE__, __LINE__, g_case.c_str(), #c);   \
        }                                                                                                \
    } while (0)

// an IDisk without a mapping: the adapter goes through read / write
class PlainDisk : public IDisk {
public:
    explicit PlainDisk(size_t n) : _data(n, 0) {}
    expected<void> read(size_t address, size_t size, static_vector<uint8_t>& data) override
    {
        if (address + size > _data.size())
            return unexpected(FsError::Disk_OutOfBounds);
        if (data.capacity() < size)
            return unexpected(FsError::Disk_InvalidRequest);
        data.resize(size);
        std::memcpy(data.data(), _data.data() + address, size);
        return {};
    }
    expected<size_t> write(size_t address, const static_vector<uint8_t>& data) override
    {
        if (address + data.size() > _data.size())
            return unexpected(FsError::Disk_OutOfBounds);
        std::memcpy(_data.data() + address, data.data(), data.size());
        return data.size();
    }
    size_t size() override { return _data.size(); }
    uint8_t* bytes() { return _data.data(); }

private:
    std::vector<uint8_t> _data;
};

constexpr size_t kDiskBytes = (size_t)1 << 18; // StackDisk<18>

using MakeDevice = std::function<std::unique_ptr<IBlockDevice>(IDisk&, std::shared_ptr<Logger>)>;

struct Pair { // the device under test and its per-block twin, each on its own disk
    std::unique_ptr<IDisk> disk[2];
    uint8_t* bytes[2];
    std::shared_ptr<Logger> log[2];
    std::unique_ptr<IBlockDevice> dev[2];
};

// is b's log the beginning of a's (whole: equal)?
static bool log_prefix(const Logger& a, const Logger& b, bool whole)
{
    if (whole ? a.events.size() != b.events.size() : a.events.size() < b.events.size())
        return false;
    for (size_t i = 0; i < b.events.size(); ++i)
        if (a.events[i].block_index != b.events[i].block_index)
            return false;
    return true;
}

// A file of n blocks on p's first disk; fail_depth / oob_depth (-1: none): the index block at that depth above
// the file's last block is damaged beyond repair / pointed past the disk.  Returns the inode record.
static ppfs_ecc_file build_file(Pair& p, std::mt19937& rng, size_t n, int fail_depth, int oob_depth, std::vector<uint8_t>& bytes)
{
    IBlockDevice& a = *p.dev[0];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize(), ipb = ds / 4;
    std::memset(p.bytes[0], 0, kDiskBytes);
    // the tree's nodes by (depth, id): the walk over all n blocks finds them
    std::map<std::vector<uint64_t>, block_index_t> node; // key: segment, slots above
    std::vector<std::vector<uint64_t>> order;
    for (size_t j = 0; j < n; ++j) {
        const auto fp = IBlockDevice::file_path(j, ipb);
        for (unsigned d = 0; d < fp.segment; ++d) {
            std::vector<uint64_t> key { fp.segment };
            key.insert(key.end(), fp.slot, fp.slot + d);
            if (!node.count(key)) {
                node[key] = 0;
                order.push_back(key);
            }
        }
    }
    const size_t total = n + order.size() + 3;
    EXPECT_TRUE(total <= a.numOfBlocks());
    std::vector<block_index_t> perm(total);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    for (size_t k = 0; k < order.size(); ++k)
        node[order[k]] = perm[n + k];
    ppfs_ecc_file f {};
    f.file_size = (uint32_t)((n - 1) * ds + (ds + 1) / 2);
    std::map<std::vector<uint64_t>, std::vector<uint8_t>> entries;
    for (const auto& key : order)
        entries[key].assign(4 * ipb, 0);
    auto put = [&](const std::vector<uint64_t>& parent, uint64_t slot, block_index_t v) {
        uint8_t* e = entries[parent].data() + 4 * slot;
        for (int q = 0; q < 4; ++q)
            e[q] = (uint8_t)(v >> (8 * q));
    };
    const auto last = IBlockDevice::file_path(n - 1, ipb);
    const block_index_t past = (block_index_t)a.numOfBlocks() + 9;
    for (const auto& key : order) {
        block_index_t v = node[key];
        // the node at depth oob_depth on the last block's path
        std::vector<uint64_t> on_path { last.segment };
        on_path.insert(on_path.end(), last.slot, last.slot + (key.size() - 1));
        if (oob_depth >= 0 && key.size() == (size_t)oob_depth + 1 && key == on_path)
            v = past;
        if (key.size() == 1)
            (key[0] == 1 ? f.indirect : key[0] == 2 ? f.doubly_indirect : f.trebly_indirect) = v;
        else
            put(std::vector<uint64_t>(key.begin(), key.end() - 1), key.back(), v);
    }
    bytes.assign(n * ds, 0);
    for (auto& x : bytes)
        x = (uint8_t)rng();
    for (size_t j = 0; j < n; ++j) {
        const auto fp = IBlockDevice::file_path(j, ipb);
        if (fp.segment == 0)
            f.direct[j] = perm[j];
        else {
            std::vector<uint64_t> key { fp.segment };
            key.insert(key.end(), fp.slot, fp.slot + fp.segment - 1);
            put(key, fp.slot[fp.segment - 1], perm[j]);
        }
        static_vector<uint8_t> v(bytes.data() + j * ds, ds, ds);
        EXPECT_TRUE((bool)a.writeBlock(v, DataLocation((int)perm[j], 0)));
    }
    for (const auto& key : order) { // _writeIndexBlock: the entries at {block, 0}
        auto& e = entries[key];
        static_vector<uint8_t> v(e.data(), e.size(), e.size());
        EXPECT_TRUE((bool)a.writeBlock(v, DataLocation((int)node[key], 0)));
    }
    // damage: one or two flipped bits in every third data block and every second index block; the failing node
    // gets a byte of noise in each eighth of the block (beyond every codec here but Reed-Solomon, which never
    // reports a failure)
    for (size_t j = 0; j < n; j += 3)
        for (size_t k = 0; k < 1 + j % 2; ++k)
            p.bytes[0][perm[j] * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    for (size_t k = 0; k < order.size(); k += 2)
        p.bytes[0][node[order[k]] * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    if (fail_depth >= 0 && last.segment > (unsigned)fail_depth) {
        std::vector<uint64_t> key { last.segment };
        key.insert(key.end(), last.slot, last.slot + fail_depth);
        uint8_t* row = p.bytes[0] + (size_t)node[key] * raw;
        for (size_t q = 0; q < 8; ++q)
            row[q * raw / 8 + rng() % std::max<size_t>(1, raw / 8)] ^= (uint8_t)(1 + rng() % 255);
    }
    return f;
}

// after one call on both devices: the logs and the disks.  start: the disks before the call.
static void compare(Pair& p, const std::vector<uint8_t>& start, bool failed)
{
    const size_t raw = p.dev[0]->rawBlockSize();
    EXPECT_TRUE(log_prefix(*p.log[0], *p.log[1], !failed));
    if (!failed) {
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
        return;
    }
    bool same = true; // every block the loop changed holds the same bytes on both disks
    for (size_t b = 0; b < kDiskBytes / raw; ++b)
        if (std::memcmp(p.bytes[1] + b * raw, start.data() + b * raw, raw) != 0)
            same = same && std::memcmp(p.bytes[0] + b * raw, p.bytes[1] + b * raw, raw) == 0;
    EXPECT_TRUE(same);
}

static void reset(Pair& p, const std::vector<uint8_t>& start)
{
    for (int k = 0; k < 2; ++k) {
        std::memcpy(p.bytes[k], start.data(), kDiskBytes);
        p.log[k]->events.clear();
    }
}

// brief: the whole file only (the damaged trees, whose every range ends at the same block); returns whether any
// call met a failing block
static bool run_file(Pair& p, std::mt19937& rng, size_t n, int fail_depth, int oob_depth, bool brief)
{
    IBlockDevice& a = *p.dev[0];
    IBlockDevice& b = *p.dev[1];
    const size_t ds = a.dataSize();
    std::vector<uint8_t> bytes;
    const ppfs_ecc_file f = build_file(p, rng, n, fail_depth, oob_depth, bytes);
    const std::vector<uint8_t> start(p.bytes[0], p.bytes[0] + kDiskBytes);
    bool any_failed = false;

    const std::pair<uint64_t, size_t> ranges[] = { { 0, n }, { 5, 1 }, { 11, std::min<size_t>(n - 11, 4) }, { n / 2, n - n / 2 },
        { n - 1, 1 }, { n - 1, 2 }, { 3, 0 } };
    for (const auto& [first, count] : ranges) {
        if (brief && count != n)
            continue;
        reset(p, start);
        std::vector<block_index_t> ia(count + 1, 0xABABABABu), ib(count + 1, 0xABABABABu);
        std::vector<uint8_t> ea(count + 1, 0xEE), eb(count + 1, 0xEE);
        auto ra = a.fileBlocks(f, first, count, ia.data(), ea.data());
        auto rb = b.IBlockDevice::fileBlocks(f, first, count, ib.data(), eb.data()); // the per-block loop
        EXPECT_TRUE((bool)ra == (bool)rb && (ra || ra.error() == rb.error()));
        EXPECT_TRUE(ea == eb);
        size_t good = 0;
        while (good < count && eb[good] == 0)
            ++good;
        EXPECT_TRUE(std::equal(ia.begin(), ia.begin() + good, ib.begin()) && ia[count] == 0xABABABABu);
        EXPECT_TRUE((bool)rb == (good == count));
        compare(p, start, !rb);
        any_failed = any_failed || (!rb && first + count <= n);
    }
    const size_t size = f.file_size;
    const std::pair<size_t, size_t> reads[] = { { 0, size }, { 0, size + 100 }, { 3, 1 }, { 7 * ds + 3, 20 * ds }, { size - 1, 1 },
        { size - std::min<size_t>(size, 2 * ds) - 1, 5 * ds }, { size, 1 }, { 9, 0 } };
    for (const auto& [offset, nbytes] : reads) {
        if (brief && nbytes != size && nbytes != 20 * ds)
            continue;
        reset(p, start);
        const size_t cap = std::min(nbytes, size) + 16;
        std::vector<uint8_t> oa(cap, 0xCD), ob(cap, 0xCD);
        size_t da = 77, db = 77;
        auto ra = a.readFile(f, offset, nbytes, oa.data(), &da);
        auto rb = b.IBlockDevice::readFile(f, offset, nbytes, ob.data(), &db); // the per-block loop
        EXPECT_TRUE((bool)ra == (bool)rb && (ra ? *ra == *rb : ra.error() == rb.error()));
        EXPECT_TRUE(da == db);
        EXPECT_TRUE(std::equal(oa.begin(), oa.begin() + db, ob.begin()));
        if (rb) {
            EXPECT_TRUE(*rb == (offset < size ? std::min(nbytes, size - offset) : 0) && db == *rb);
            EXPECT_TRUE(std::all_of(oa.begin() + db, oa.end(), [](uint8_t x) { return x == 0xCD; }));
        }
        compare(p, start, !rb);
        any_failed = any_failed || (!rb && offset < size);
    }
    (void)bytes;
    return any_failed;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    // the number of file blocks reaches every level of each codec's tree that fits the disk of 256 KiB
    struct Codec {
        const char* name;
        MakeDevice make;
        size_t n;
        bool can_fail; // the codec reports a block beyond its capability (Reed-Solomon's decode never does)
    };
    const std::vector<Codec> codecs = {
        { "rs512t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 512, 3, l); }, 400, false },
        { "rs64t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 64, 3, l); }, 260, false },
        { "crc64",
            [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<CrcBlockDevice>(CrcPolynomial::MsgImplicit(0x9960034c), d, 64, l); },
            330, true },
        { "hamming256", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<HammingBlockDevice>(8, d, l); }, 300, true },
        { "parity3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ParityBlockDevice>(3, d, l); }, 10, true },
    };
    std::mt19937 rng(20250101);
    for (const Codec& c : codecs) {
        for (const char* kind : { "stack", "file", "plain" }) {
            g_case = std::string(c.name) + "/" + kind;
            Pair p;
            bool ok = true;
            for (int k = 0; k < 2; ++k) {
                if (kind[0] == 's') {
                    auto d = std::make_unique<StackDisk<18>>();
                    p.bytes[k] = d->mapped();
                    p.disk[k] = std::move(d);
                } else if (kind[0] == 'f') {
                    auto d = std::make_unique<MappedFileDisk>();
                    ok = ok && (bool)d->create(dir + "/" + c.name + "_" + std::to_string(k) + ".img", kDiskBytes);
                    p.bytes[k] = d->mapped();
                    p.disk[k] = std::move(d);
                } else {
                    auto d = std::make_unique<PlainDisk>(kDiskBytes);
                    p.bytes[k] = d->bytes();
                    p.disk[k] = std::move(d);
                }
                p.log[k] = std::make_shared<Logger>();
            }
            EXPECT_TRUE(ok && p.bytes[0] && p.bytes[1]);
            if (!ok || !p.bytes[0] || !p.bytes[1])
                continue;
            for (int k = 0; k < 2; ++k)
                p.dev[k] = c.make(*p.disk[k], p.log[k]);
            (void)run_file(p, rng, c.n, -1, -1, false);
            const unsigned depth = IBlockDevice::file_path(c.n - 1, p.dev[0]->dataSize() / 4).segment;
            for (unsigned d = 0; d < depth && d < 3; ++d) {
                g_case = std::string(c.name) + "/" + kind + "/depth" + std::to_string(d);
                if (c.can_fail)
                    EXPECT_TRUE(run_file(p, rng, c.n, (int)d, -1, true)); // an index block beyond repair
                EXPECT_TRUE(run_file(p, rng, c.n, -1, (int)d, true));     // a pointer past the disk
            }
            p.dev[0].reset(); // devices before their disks
            p.dev[1].reset();
        }
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail)
        return 1;
    std::printf("ALL PASSED\n");
    return 0;
}
