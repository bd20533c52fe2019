// test_block_files.cpp -- readFiles of the C++ adapter (include/ppfs_gpu/block_device.hpp) on the GPU,
// differentially: one readFiles call on one device is compared with the loop over readFile, which is its
// definition, on a second device over a copy of the disk -- per file the result, the bytes and the delivered
// count, then the whole disk image and the correction log in order.  One variant damages a file in mid-batch
// beyond repair.  Several fragmented files share the disk, written through the adapter the way the reference
// writes them (index blocks by a write of their entries at {block, 0}, data blocks whole), all placed by one
// seeded permutation.
// Disks: StackDisk and MappedFileDisk (mapped: engine calls on the image) and a plain in-memory disk without a
// mapping (the per-block loop).
//
// usage: test_block_files <directory for the file-backed disks>
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

struct Pair { // the device under test and its twin, each on its own disk
    std::unique_ptr<IDisk> disk[2];
    uint8_t* bytes[2];
    std::shared_ptr<Logger> log[2];
    std::unique_ptr<IBlockDevice> dev[2];
};

// Files of sizes[f] blocks on p's first disk (0: an empty file); fail_file (-1: none): its first index block, or
// its first data block when it has no tree, gets a byte of noise in each eighth of the block.
static std::vector<ppfs_ecc_file> build_files(Pair& p, std::mt19937& rng, const std::vector<size_t>& sizes, int fail_file)
{
    IBlockDevice& a = *p.dev[0];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize(), ipb = ds / 4;
    std::memset(p.bytes[0], 0, kDiskBytes);
    using Key = std::vector<uint64_t>; // segment, slots above
    std::vector<std::vector<Key>> order(sizes.size());
    size_t total = 3;
    for (size_t f = 0; f < sizes.size(); ++f) {
        std::map<Key, int> seen;
        for (size_t j = 0; j < sizes[f]; ++j) {
            const auto fp = IBlockDevice::file_path(j, ipb);
            for (unsigned d = 0; d < fp.segment; ++d) {
                Key key { fp.segment };
                key.insert(key.end(), fp.slot, fp.slot + d);
                if (!seen.count(key)) {
                    seen[key] = 1;
                    order[f].push_back(key);
                }
            }
        }
        total += sizes[f] + order[f].size();
    }
    EXPECT_TRUE(total <= a.numOfBlocks());
    std::vector<block_index_t> perm(total);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<ppfs_ecc_file> files(sizes.size());
    size_t at = 0;
    for (size_t f = 0; f < sizes.size(); ++f) {
        const size_t n = sizes[f];
        ppfs_ecc_file& file = files[f];
        file = ppfs_ecc_file {};
        file.file_size = n ? (uint32_t)((n - 1) * ds + (ds + 1) / 2) : 0;
        const block_index_t* data = perm.data() + at;
        std::map<Key, block_index_t> node;
        std::map<Key, std::vector<uint8_t>> entries;
        for (size_t k = 0; k < order[f].size(); ++k) {
            node[order[f][k]] = perm[at + n + k];
            entries[order[f][k]].assign(4 * ipb, 0);
        }
        at += n + order[f].size();
        auto put = [&](const Key& parent, uint64_t slot, block_index_t v) {
            uint8_t* e = entries[parent].data() + 4 * slot;
            for (int q = 0; q < 4; ++q)
                e[q] = (uint8_t)(v >> (8 * q));
        };
        for (const Key& key : order[f]) {
            if (key.size() == 1)
                (key[0] == 1 ? file.indirect : key[0] == 2 ? file.doubly_indirect : file.trebly_indirect) = node[key];
            else
                put(Key(key.begin(), key.end() - 1), key.back(), node[key]);
        }
        std::vector<uint8_t> block(ds);
        for (size_t j = 0; j < n; ++j) {
            const auto fp = IBlockDevice::file_path(j, ipb);
            if (fp.segment == 0)
                file.direct[j] = data[j];
            else {
                Key key { fp.segment };
                key.insert(key.end(), fp.slot, fp.slot + fp.segment - 1);
                put(key, fp.slot[fp.segment - 1], data[j]);
            }
            for (auto& x : block)
                x = (uint8_t)rng();
            static_vector<uint8_t> v(block.data(), ds, ds);
            EXPECT_TRUE((bool)a.writeBlock(v, DataLocation((int)data[j], 0)));
        }
        for (const Key& key : order[f]) { // _writeIndexBlock: the entries at {block, 0}
            auto& e = entries[key];
            static_vector<uint8_t> v(e.data(), e.size(), e.size());
            EXPECT_TRUE((bool)a.writeBlock(v, DataLocation((int)node[key], 0)));
        }
        // damage: one or two flipped bits in every third data block and every second index block
        for (size_t j = 0; j < n; j += 3)
            for (size_t k = 0; k < 1 + j % 2; ++k)
                p.bytes[0][data[j] * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
        for (size_t k = 0; k < order[f].size(); k += 2)
            p.bytes[0][node[order[f][k]] * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
        if ((int)f == fail_file && n) {
            uint8_t* row = p.bytes[0] + (size_t)(order[f].empty() ? data[0] : node[order[f][0]]) * raw;
            for (size_t q = 0; q < 8; ++q)
                row[q * raw / 8 + rng() % std::max<size_t>(1, raw / 8)] ^= (uint8_t)(1 + rng() % 255);
        }
    }
    return files;
}

// returns whether any read of the batch failed on a block
static bool run_batch(Pair& p, const std::vector<ppfs_ecc_file>& files, const std::vector<std::pair<size_t, size_t>>& ranges,
    const std::vector<uint8_t>& start)
{
    for (int k = 0; k < 2; ++k) {
        std::memcpy(p.bytes[k], start.data(), kDiskBytes);
        p.log[k]->events.clear();
    }
    const size_t n = files.size();
    std::vector<std::vector<uint8_t>> oa(n), ob(n);
    std::vector<IBlockDevice::FileRead> reads(n);
    for (size_t f = 0; f < n; ++f) {
        oa[f].assign(std::min<size_t>(ranges[f].second, files[f].file_size) + 16, 0xCD);
        ob[f] = oa[f];
        reads[f] = IBlockDevice::FileRead { files[f], ranges[f].first, ranges[f].second, oa[f].data(), false, FsError {}, 77, 77 };
    }
    p.dev[0]->readFiles(reads.data(), n);
    bool any_failed = false;
    for (size_t f = 0; f < n; ++f) { // the loop over readFile
        size_t db = 77;
        auto rb = p.dev[1]->readFile(files[f], ranges[f].first, ranges[f].second, ob[f].data(), &db);
        const IBlockDevice::FileRead& ra = reads[f];
        EXPECT_TRUE(ra.ok == (bool)rb && (rb ? ra.bytes == *rb : ra.error == rb.error()));
        EXPECT_TRUE(ra.delivered == db);
        EXPECT_TRUE(oa[f] == ob[f]);
        if (rb)
            EXPECT_TRUE(std::all_of(oa[f].begin() + db, oa[f].end(), [](uint8_t x) { return x == 0xCD; }));
        any_failed = any_failed || (!rb && ranges[f].first < files[f].file_size);
    }
    EXPECT_TRUE(p.log[0]->events.size() == p.log[1]->events.size());
    for (size_t i = 0; i < std::min(p.log[0]->events.size(), p.log[1]->events.size()); ++i)
        EXPECT_TRUE(p.log[0]->events[i].block_index == p.log[1]->events[i].block_index);
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    return any_failed;
}

static bool run_files(Pair& p, std::mt19937& rng, const std::vector<size_t>& sizes, int fail_file)
{
    const std::vector<ppfs_ecc_file> files = build_files(p, rng, sizes, fail_file);
    const std::vector<uint8_t> start(p.bytes[0], p.bytes[0] + kDiskBytes);
    const size_t ds = p.dev[0]->dataSize();
    std::vector<std::pair<size_t, size_t>> whole, mid, odd;
    for (size_t f = 0; f < files.size(); ++f) {
        const size_t size = files[f].file_size;
        whole.push_back({ 0, size });
        const size_t off = size > 14 * ds ? 13 * ds + 5 : size > 10 ? 3 : 0;
        mid.push_back({ off, size - off > 5 ? size - off - 2 : size - off });
        odd.push_back(f == 2 ? std::make_pair(size, (size_t)1) : f == 3 ? std::make_pair((size_t)9, (size_t)0) : std::make_pair((size_t)0, size + 100));
    }
    bool any_failed = run_batch(p, files, whole, start);
    any_failed = run_batch(p, files, mid, start) || any_failed;
    (void)run_batch(p, files, odd, start);
    (void)run_batch(p, {}, {}, start);
    return any_failed;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    struct Codec {
        const char* name;
        MakeDevice make;
        std::vector<size_t> sizes; // the failing file is number 3, in mid-batch
        bool can_fail;             // a block of noise is reported as beyond the code's capability (Reed-Solomon's decode never
                                   // reports one; a 3-byte parity block of noise may pass, and its flipped bits fail anyway)
    };
    const std::vector<size_t> usual = { 5, 0, 13, 200, 1, 90, 12 };
    const std::vector<Codec> codecs = {
        { "rs512t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 512, 3, l); }, usual, false },
        { "rs64t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 64, 3, l); }, usual, false },
        { "crc64",
            [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<CrcBlockDevice>(CrcPolynomial::MsgImplicit(0x9960034c), d, 64, l); },
            usual, true },
        { "hamming256", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<HammingBlockDevice>(8, d, l); }, usual, true },
        { "parity3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ParityBlockDevice>(3, d, l); }, { 5, 0, 12, 9, 1 }, false },
    };
    std::mt19937 rng(20250303);
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
            (void)run_files(p, rng, c.sizes, -1);
            if (c.can_fail) {
                g_case += "/failing";
                EXPECT_TRUE(run_files(p, rng, c.sizes, 3)); // a file in mid-batch damaged beyond repair
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
