// test_block_file_write.cpp -- writeFile / writeFiles of the C++ adapter (include/ppfs_gpu/block_device.hpp) on
// the GPU, differentially: one writeFiles call (and one writeFile per file) on one device is compared with the
// per-block loop IBlockDevice::writeFile, which is its definition, on a second device over a copy of the disk --
// per file the result and the written count, then the disk image and the correction log.  Where no block fails
// image and log are equal; where one fails, the loop stops there while the engine attempts every block, so the
// rows the loop touched are compared and the loop's log must be a prefix of the file's.  One variant damages a
// file in mid-batch beyond repair.  Several fragmented files share the disk, written through the adapter the way
// the reference writes them, all placed by one seeded permutation.
// Disks: StackDisk and MappedFileDisk (mapped: engine calls on the image) and a plain in-memory disk without a
// mapping (the per-block loop).
//
// usage: test_block_file_write <directory for the file-backed disks>
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

// single: one writeFile per file in place of one writeFiles.  Returns whether any write failed on a block.
static bool run_batch(Pair& p, const std::vector<ppfs_ecc_file>& files, const std::vector<std::pair<size_t, size_t>>& ranges,
    const std::vector<uint8_t>& start, std::mt19937& rng, bool single)
{
    for (int k = 0; k < 2; ++k) {
        std::memcpy(p.bytes[k], start.data(), kDiskBytes);
        p.log[k]->events.clear();
    }
    const size_t n = files.size(), raw = p.dev[0]->rawBlockSize();
    std::vector<std::vector<uint8_t>> in(n);
    std::vector<IBlockDevice::FileWrite> writes(n);
    for (size_t f = 0; f < n; ++f) {
        in[f].resize(ranges[f].second + 1);
        for (auto& x : in[f])
            x = (uint8_t)rng();
        writes[f] = IBlockDevice::FileWrite { files[f], ranges[f].first, in[f].data(), ranges[f].second, false, FsError {}, 77, 77 };
    }
    if (single)
        for (size_t f = 0; f < n; ++f) {
            IBlockDevice::FileWrite& w = writes[f];
            auto r = p.dev[0]->writeFile(w.file, w.offset, w.in, w.n, &w.written);
            w.ok = (bool)r;
            w.error = r ? FsError {} : r.error();
            w.bytes = r ? *r : 0;
        }
    else
        p.dev[0]->writeFiles(writes.data(), n);
    bool any_failed = false;
    std::vector<uint8_t> before(p.bytes[1], p.bytes[1] + kDiskBytes);
    size_t log_at = 0; // where this file's events start in the engine's log
    bool aligned = true;
    for (size_t f = 0; f < n; ++f) { // the per-block loop, which is the definition
        const size_t events_before = p.log[1]->events.size();
        size_t wb = 77;
        auto rb = p.dev[1]->IBlockDevice::writeFile(files[f], ranges[f].first, in[f].data(), ranges[f].second, &wb);
        const IBlockDevice::FileWrite& wa = writes[f];
        EXPECT_TRUE(wa.ok == (bool)rb && (rb ? wa.bytes == *rb : wa.error == rb.error()));
        EXPECT_TRUE(wa.written == wb);
        const bool in_file = ranges[f].second && ranges[f].first + ranges[f].second <= files[f].file_size;
        EXPECT_TRUE(in_file || !ranges[f].second || (!rb && rb.error() == FsError::FileIO_OutOfBounds && wb == 0));
        const bool failed = !rb && in_file;
        any_failed = any_failed || failed;
        // the loop's events of this file are the first of the engine's events of this file
        const size_t mine = p.log[1]->events.size() - events_before;
        if (aligned) {
            EXPECT_TRUE(log_at + mine <= p.log[0]->events.size());
            for (size_t i = 0; i < mine && log_at + i < p.log[0]->events.size(); ++i)
                EXPECT_TRUE(p.log[0]->events[log_at + i].block_index == p.log[1]->events[events_before + i].block_index);
            log_at += mine;
        }
        aligned = aligned && !failed; // the engine logged blocks after the failing one: later files start further on
    }
    if (!any_failed) {
        EXPECT_TRUE(p.log[0]->events.size() == p.log[1]->events.size());
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    }
    // every row the loop changed holds the same bytes on the engine's disk (all of them when nothing failed)
    for (size_t b = 0; b + raw <= kDiskBytes; b += raw)
        if (std::memcmp(p.bytes[1] + b, before.data() + b, raw) != 0)
            EXPECT_TRUE(std::memcmp(p.bytes[0] + b, p.bytes[1] + b, raw) == 0);
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
        // one byte past the end, an offset at the end, an empty write, the last byte alone
        odd.push_back(f == 2 ? std::make_pair((size_t)1, size) : f == 3 ? std::make_pair((size_t)9, (size_t)0)
                : f == 4     ? std::make_pair(size, (size_t)1)
                             : std::make_pair(size ? size - 1 : 0, size ? (size_t)1 : (size_t)0));
    }
    bool any_failed = run_batch(p, files, whole, start, rng, false);
    any_failed = run_batch(p, files, mid, start, rng, false) || any_failed;
    any_failed = run_batch(p, files, mid, start, rng, true) || any_failed;
    (void)run_batch(p, files, odd, start, rng, false);
    (void)run_batch(p, {}, {}, start, rng, false);
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
