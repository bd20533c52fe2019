// test_block_list.cpp -- readBlockList / writeBlockList of the C++ adapter
// (include/ppfs_gpu/block_device.hpp) on the GPU, differentially: every list call on one device is
// compared with the per-block readBlock / writeBlock loop, in list order, on a second device over a
// copy of the disk -- payloads, per-entry errors, the whole disk image and the correction log.
// Disks: StackDisk and MappedFileDisk (the image is mapped: one engine list call on it) and a plain
// in-memory disk without a mapping (rows read and written through IDisk).  Lists: distinct blocks in
// a scattered order, a list with repeated blocks, and one with blocks off the disk.
//
// usage: test_block_list <directory for the file-backed disks>
// Exit status 0 and "ALL PASSED" on success.  Needs a GPU (the adapter has no CPU fallback).
#include "ppfs_gpu/block_device.hpp"

#include <cstdio>
#include <functional>
#include <memory>
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

constexpr size_t kBlocks = 96;
constexpr size_t kDiskBytes = (size_t)1 << 16; // StackDisk<16>

using MakeDevice = std::function<std::unique_ptr<IBlockDevice>(IDisk&, std::shared_ptr<Logger>)>;

struct Pair { // the device under test and its per-block twin, each on its own disk
    std::unique_ptr<IDisk> disk[2];
    uint8_t* bytes[2];
    std::shared_ptr<Logger> log[2];
    std::unique_ptr<IBlockDevice> dev[2];
};

static bool same_log(const Logger& a, const Logger& b)
{
    if (a.events.size() != b.events.size())
        return false;
    for (size_t i = 0; i < a.events.size(); ++i)
        if (a.events[i].block_index != b.events[i].block_index)
            return false;
    return true;
}

static void run_lists(Pair& p, std::mt19937& rng)
{
    IBlockDevice& a = *p.dev[0];
    IBlockDevice& b = *p.dev[1];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize();
    EXPECT_TRUE(raw > 0 && kBlocks * raw <= kDiskBytes);
    if (!raw || kBlocks * raw > kDiskBytes)
        return;
    const block_index_t off_disk = (block_index_t)a.numOfBlocks();
    // a written disk with damage of every weight the codec meets
    std::vector<uint8_t> payloads(kBlocks * ds), err(kBlocks);
    for (auto& x : payloads)
        x = (uint8_t)rng();
    EXPECT_TRUE((bool)a.writeBlocks(0, kBlocks, payloads.data(), err.data()));
    for (size_t blk = 0; blk < kBlocks; blk += 3)
        for (size_t k = 0; k < 1 + blk % 3; ++k)
            p.bytes[0][blk * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    std::memcpy(p.bytes[1], p.bytes[0], kDiskBytes);
    p.log[0]->events.clear();
    p.log[1]->events.clear();

    // 41 distinct blocks: 0..15, the last, 24 others outside 40..49, shuffled
    std::vector<block_index_t> base;
    for (block_index_t i = 0; i < 16; ++i)
        base.push_back(i);
    base.push_back((block_index_t)kBlocks - 1);
    std::vector<block_index_t> pool;
    for (block_index_t i = 16; i < kBlocks - 1; ++i)
        if (i < 40 || i >= 50)
            pool.push_back(i);
    std::shuffle(pool.begin(), pool.end(), rng);
    base.insert(base.end(), pool.begin(), pool.begin() + 24);
    std::shuffle(base.begin(), base.end(), rng);

    std::vector<std::vector<block_index_t>> lists(3, base);
    lists[1].insert(lists[1].begin() + 9, { base[3], base[3] }); // repeats, adjacent and far apart
    lists[1].push_back(base[0]);
    lists[2].insert(lists[2].begin() + 5, { off_disk, off_disk + 7 }); // off the disk

    for (const auto& ix : lists) {
        const size_t n = ix.size();
        std::vector<uint8_t> out(n * ds, 0xEE), e(n, 0xEE), one(ds);
        EXPECT_TRUE((bool)a.readBlockList(ix.data(), n, out.data(), e.data()));
        for (size_t k = 0; k < n; ++k) {
            static_vector<uint8_t> v(one.data(), ds, 0);
            auto r = b.readBlock(DataLocation((int)ix[k], 0), ds, v);
            EXPECT_TRUE(e[k] == (r ? 0 : (uint8_t)r.error()));
            if (r)
                EXPECT_TRUE(std::memcmp(out.data() + k * ds, one.data(), ds) == 0);
        }
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
        EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));

        for (size_t k = 0; k < n; k += 4) // fresh damage for the writes' read-modify-write
            if (ix[k] < kBlocks)
                p.bytes[0][ix[k] * raw + rng() % raw] ^= 0x10;
        std::memcpy(p.bytes[1], p.bytes[0], kDiskBytes);
        std::vector<uint8_t> fresh(n * ds);
        for (auto& x : fresh)
            x = (uint8_t)rng();
        std::fill(e.begin(), e.end(), 0xEE);
        EXPECT_TRUE((bool)a.writeBlockList(ix.data(), n, fresh.data(), e.data()));
        for (size_t k = 0; k < n; ++k) {
            static_vector<uint8_t> v(fresh.data() + k * ds, ds, ds);
            auto r = b.writeBlock(v, DataLocation((int)ix[k], 0));
            EXPECT_TRUE(e[k] == (r ? 0 : (uint8_t)r.error()));
        }
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
        EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));
    }
}

// readBlockList / writeBlockList with err == nullptr == the per-block loop: payloads (zeros for a failed
// entry), the disk image and the log in order.  The disk is 8 blocks, mapped or not, one with a single
// flipped bit and one damaged past what the codec corrects; the list adds an index past the disk and a
// repeated one, so the calls meet ok, corrected, failed and out of bounds with nowhere to report them.
class SmallDisk : public PlainDisk {
public:
    SmallDisk(size_t n, bool map) : PlainDisk(n), _map(map) {}
    uint8_t* mapped() override { return _map ? bytes() : nullptr; }

private:
    bool _map;
};

static void run_null_outputs(const std::string& name, const MakeDevice& make, size_t raw)
{
    constexpr size_t NB = 8;
    std::mt19937 rng(20240611 + (unsigned)raw); // its own: the other cases' draws stay what they were
    const bool rs = name.compare(0, 2, "rs") == 0, corrects = rs || name.compare(0, 7, "hamming") == 0;
    for (bool map : { true, false }) {
        g_case = name + (map ? "/null-outputs/mapped" : "/null-outputs/plain");
        SmallDisk da(NB * raw, map), db(NB * raw, map);
        auto la = std::make_shared<Logger>(), lb = std::make_shared<Logger>();
        auto a = make(da, la), b = make(db, lb);
        const size_t ds = a->dataSize();
        std::vector<uint8_t> payloads(NB * ds), err(NB);
        for (auto& x : payloads)
            x = (uint8_t)rng();
        EXPECT_TRUE((bool)a->writeBlocks(0, NB, payloads.data(), err.data()));
        std::vector<uint8_t> bad(da.bytes(), da.bytes() + NB * raw);
        bad[2 * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
        const size_t nbad = rs ? 5 : 2; // distinct bytes: past t = 3, past one bit
        for (size_t k = 0; k < nbad; ++k)
            bad[5 * raw + k * (raw / nbad)] ^= (uint8_t)(1u << (rng() % 8));
        auto damaged = [&]() {
            std::memcpy(da.bytes(), bad.data(), bad.size());
            std::memcpy(db.bytes(), bad.data(), bad.size());
            la->events.clear();
            lb->events.clear();
        };
        const std::vector<block_index_t> ix = { 4, 2, (block_index_t)a->numOfBlocks(), 5, 2, 0 };
        const size_t n = ix.size();
        size_t failed = 0;

        damaged();
        std::vector<uint8_t> out(n * ds, 0xEE), one(ds), zeros(ds, 0);
        EXPECT_TRUE((bool)a->readBlockList(ix.data(), n, out.data(), nullptr));
        for (size_t k = 0; k < n; ++k) {
            static_vector<uint8_t> v(one.data(), ds, 0);
            auto r = b->readBlock(DataLocation((int)ix[k], 0), ds, v);
            failed += !r;
            EXPECT_TRUE(std::memcmp(out.data() + k * ds, r ? one.data() : zeros.data(), ds) == 0);
        }
        EXPECT_TRUE(std::memcmp(da.bytes(), db.bytes(), NB * raw) == 0);
        EXPECT_TRUE(same_log(*la, *lb));
        // off the disk, and the damage -- except for RS, which never fails a block: it logs what its decoder made of it
        EXPECT_TRUE(failed >= (rs || name == "raw255" ? 1u : 2u));
        EXPECT_TRUE(!corrects || lb->events.size() >= 1);

        damaged();
        std::vector<uint8_t> fresh(n * ds);
        for (auto& x : fresh)
            x = (uint8_t)rng();
        EXPECT_TRUE((bool)a->writeBlockList(ix.data(), n, fresh.data(), nullptr));
        for (size_t k = 0; k < n; ++k) {
            static_vector<uint8_t> v(fresh.data() + k * ds, ds, ds);
            (void)b->writeBlock(v, DataLocation((int)ix[k], 0));
        }
        EXPECT_TRUE(std::memcmp(da.bytes(), db.bytes(), NB * raw) == 0);
        EXPECT_TRUE(same_log(*la, *lb));
        EXPECT_TRUE(!corrects || lb->events.size() >= 1);
    }
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::vector<std::pair<const char*, MakeDevice>> codecs = {
        { "rs512t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 512, 3, l); } },
        { "rs64t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 64, 3, l); } },
        { "crc64", [](IDisk& d, std::shared_ptr<Logger> l) {
             return std::make_unique<CrcBlockDevice>(CrcPolynomial::MsgImplicit(0x9960034c), d, 64, l);
         } },
        { "hamming256", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<HammingBlockDevice>(8, d, l); } },
        { "parity3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ParityBlockDevice>(3, d, l); } },
        { "raw255", [](IDisk& d, std::shared_ptr<Logger>) { return std::make_unique<RawBlockDevice>(255, d); } },
    };
    std::mt19937 rng(20240611);
    for (const auto& [name, make] : codecs) {
        for (const char* kind : { "stack", "file", "plain" }) {
            g_case = std::string(name) + "/" + kind;
            Pair p;
            bool ok = true;
            for (int k = 0; k < 2; ++k) {
                if (kind[0] == 's') {
                    auto d = std::make_unique<StackDisk<16>>();
                    p.bytes[k] = d->mapped();
                    p.disk[k] = std::move(d);
                } else if (kind[0] == 'f') {
                    auto d = std::make_unique<MappedFileDisk>();
                    ok = ok && (bool)d->create(dir + "/" + name + "_" + std::to_string(k) + ".img", kDiskBytes);
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
                p.dev[k] = make(*p.disk[k], p.log[k]);
            run_lists(p, rng);
            if (kind[0] == 's' && p.dev[0]->rawBlockSize()) // once per codec, on 8-block disks of its own
                run_null_outputs(name, make, p.dev[0]->rawBlockSize());
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
