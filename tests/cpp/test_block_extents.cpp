// test_block_extents.cpp -- readExtents / writeExtents of the C++ adapter
// (include/ppfs_gpu/block_device.hpp) on the GPU, differentially: every extent call on one device is
// compared with the per-block readBlock / writeBlock loop, in list order, on a second device over a
// copy of the disk -- the packed bytes, per-entry errors, the whole disk image and the correction log.
// Disks: StackDisk (the image is mapped: one engine call on it) and a plain in-memory disk without a
// mapping (the default loop).  Batches: a file walk (file_extents) and a batch of segment shapes with a
// block named again, two writes into one block, and entries off the disk, past dataSize() and past
// the packed buffer.
//
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
constexpr size_t kGuard = 64;

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

static void damage(Pair& p, size_t raw, std::mt19937& rng)
{
    for (size_t blk = 0; blk < kBlocks; blk += 3)
        for (size_t k = 0; k < 1 + blk % 3; ++k)
            p.bytes[0][blk * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    std::memcpy(p.bytes[1], p.bytes[0], kDiskBytes);
    p.log[0]->events.clear();
    p.log[1]->events.clear();
}

// Does the per-block loop make a call for this entry, and of how many bytes?  Restated here: the offset at
// most dataSize(), the clamped bytes inside the packed buffer, and a block index DataLocation's int holds.
static bool fits(const ppfs_ecc_extent& x, size_t ds, size_t nbytes, size_t& len)
{
    if (x.offset > ds || x.block > 0x7FFFFFFFu)
        return false;
    len = std::min<size_t>(x.length, ds - x.offset);
    return x.pos + len <= nbytes;
}

// one batch: device a's extent calls against device b's per-block loop
static void run_batch(Pair& p, const std::vector<ppfs_ecc_extent>& ext, size_t nbytes, std::mt19937& rng)
{
    IBlockDevice& a = *p.dev[0];
    IBlockDevice& b = *p.dev[1];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize(), n = ext.size();
    damage(p, raw, rng);
    // the packed buffer between guards
    std::vector<uint8_t> buf(kGuard + nbytes + kGuard, 0xA5), want(buf), e(n, 0xEE), one(ds + 1);
    EXPECT_TRUE((bool)a.readExtents(ext.data(), n, buf.data() + kGuard, nbytes, e.data()));
    for (size_t k = 0; k < n; ++k) {
        size_t len = 0;
        if (!fits(ext[k], ds, nbytes, len)) {
            EXPECT_TRUE(e[k] == (uint8_t)FsError::Disk_OutOfBounds);
            continue;
        }
        static_vector<uint8_t> v(one.data(), len, 0);
        auto r = b.readBlock(DataLocation((int)ext[k].block, ext[k].offset), len, v);
        EXPECT_TRUE(e[k] == (r ? 0 : (uint8_t)r.error()));
        if (r)
            std::memcpy(want.data() + kGuard + ext[k].pos, one.data(), len);
        else if (r.error() != FsError::Disk_OutOfBounds)
            std::memset(want.data() + kGuard + ext[k].pos, 0, len);
    }
    EXPECT_TRUE(buf == want); // the entries' bytes; the gaps and the guards as they were
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));

    damage(p, raw, rng);
    std::vector<uint8_t> fresh(nbytes);
    for (auto& x : fresh)
        x = (uint8_t)rng();
    std::fill(e.begin(), e.end(), 0xEE);
    EXPECT_TRUE((bool)a.writeExtents(ext.data(), n, fresh.data(), nbytes, e.data()));
    for (size_t k = 0; k < n; ++k) {
        size_t len = 0;
        if (!fits(ext[k], ds, nbytes, len)) {
            EXPECT_TRUE(e[k] == (uint8_t)FsError::Disk_OutOfBounds);
            continue;
        }
        static_vector<uint8_t> v(fresh.data() + ext[k].pos, len, len);
        auto r = b.writeBlock(v, DataLocation((int)ext[k].block, ext[k].offset));
        EXPECT_TRUE(e[k] == (r ? 0 : (uint8_t)r.error()));
    }
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));
    // without an error array
    EXPECT_TRUE((bool)a.readExtents(ext.data(), n, buf.data() + kGuard, nbytes, nullptr));
    EXPECT_TRUE((bool)b.readExtents(ext.data(), n, want.data() + kGuard, nbytes, nullptr));
    EXPECT_TRUE(buf == want);
}

static void run_extents(Pair& p, std::mt19937& rng)
{
    IBlockDevice& a = *p.dev[0];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize();
    EXPECT_TRUE(raw > 0 && ds > 0 && kBlocks * raw <= kDiskBytes);
    if (!raw || !ds || kBlocks * raw > kDiskBytes)
        return;
    const block_index_t off_disk = (block_index_t)a.numOfBlocks();
    std::vector<uint8_t> payloads(kBlocks * ds), err(kBlocks);
    for (auto& x : payloads)
        x = (uint8_t)rng();
    EXPECT_TRUE((bool)a.writeBlocks(0, kBlocks, payloads.data(), err.data()));

    std::vector<block_index_t> base(kBlocks);
    for (block_index_t i = 0; i < kBlocks; ++i)
        base[i] = i;
    std::shuffle(base.begin(), base.end(), rng);
    base.resize(41);

    // a file walk: from byte 1 of its first block to the middle of its last
    {
        const size_t off0 = std::min<size_t>(1, ds - 1), nbytes = (ds - off0) + 39 * ds + (ds + 1) / 2;
        const std::vector<ppfs_ecc_extent> ext = file_extents(base.data(), base.size(), off0, nbytes, ds);
        EXPECT_TRUE(ext.size() == 41 && ext.front().offset == off0 && ext.back().pos + ext.back().length == nbytes);
        run_batch(p, ext, nbytes, rng);
        const std::vector<ppfs_ecc_extent> one = file_extents(base.data(), 1, off0, 1, ds); // head = tail
        EXPECT_TRUE(one.size() == 1 && one[0].length == 1);
        run_batch(p, one, 1, rng);
    }
    // segment shapes with gaps between them, then the entries that need care
    {
        const size_t d1 = ds - 1;
        const size_t shapes[][2] = { { 0, ds }, { 0, 0 }, { ds, 0 }, { 0, 1 }, { d1, 1 }, { d1, 5 }, { std::min<size_t>(1, ds), d1 },
            { std::min<size_t>(3, ds), 16 }, { std::min<size_t>(5, ds), 17 }, { std::min<size_t>(7, ds), 15 }, { 0, ds + 9 },
            { ds / 2, 33 } };
        std::vector<ppfs_ecc_extent> ext;
        size_t pos = 0;
        for (size_t k = 0; k < base.size(); ++k) {
            const size_t off = shapes[k % 12][0], length = shapes[k % 12][1];
            ext.push_back(ppfs_ecc_extent { (uint64_t)pos, base[k], (uint16_t)off, (uint16_t)length });
            pos += std::min(length, ds - off) + 1 + k % 7;
        }
        const size_t n8 = std::min<size_t>(8, ds);
        ext.push_back(ppfs_ecc_extent { (uint64_t)pos, base[0], 0, (uint16_t)n8 });      // a block named again,
        ext.push_back(ppfs_ecc_extent { (uint64_t)pos + 8, base[0], (uint16_t)(n8 / 2), (uint16_t)n8 }); // ... and overlapped
        ext.push_back(ppfs_ecc_extent { (uint64_t)pos + 16, off_disk, 0, 4 });           // off the disk
        ext.push_back(ppfs_ecc_extent { (uint64_t)pos + 20, 0xFFFFFFFFu, 0, 4 });       // no block at all: never
                                                                                      // handed to readBlock / writeBlock
        ext.push_back(ppfs_ecc_extent { (uint64_t)pos + 24, base[1], (uint16_t)(ds + 1), 4 }); // past dataSize()
        const size_t nbytes = pos + 32;
        ext.push_back(ppfs_ecc_extent { (uint64_t)nbytes, base[2], 0, 1 });              // past the packed buffer
        ext.push_back(ppfs_ecc_extent { (uint64_t)nbytes - 1, base[3], 0, 1 });          // ... and just inside it
        run_batch(p, ext, nbytes, rng);
    }
}

// writeExtents with err == nullptr == the per-block loop: the disk image and the log in order.  The disk is
// 8 blocks, mapped or not, one with a single flipped bit and one damaged past what the codec corrects; the
// batch adds a block past the disk and a block named twice, so the call meets ok, corrected, failed and out of
// bounds with nowhere to report them.
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
    std::mt19937 rng(20241019 + (unsigned)raw); // its own: the other cases' draws stay what they were
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
        da.bytes()[2 * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
        const size_t nbad = rs ? 5 : 2; // distinct bytes: past t = 3, past one bit
        for (size_t k = 0; k < nbad; ++k)
            da.bytes()[5 * raw + k * (raw / nbad)] ^= (uint8_t)(1u << (rng() % 8));
        std::memcpy(db.bytes(), da.bytes(), NB * raw);
        la->events.clear();

        const uint16_t len = (uint16_t)std::min<size_t>(ds, 4), off = (uint16_t)std::min<size_t>(1, ds - 1);
        std::vector<ppfs_ecc_extent> ext;
        for (block_index_t blk : { 4u, 2u, (block_index_t)a->numOfBlocks(), 5u, 2u, 0u })
            ext.push_back(ppfs_ecc_extent { (uint64_t)ext.size() * 4, blk, ext.size() % 2 ? off : (uint16_t)0, len });
        std::vector<uint8_t> fresh(ext.size() * 4);
        for (auto& x : fresh)
            x = (uint8_t)rng();
        EXPECT_TRUE((bool)a->writeExtents(ext.data(), ext.size(), fresh.data(), fresh.size(), nullptr));
        size_t failed = 0;
        for (const ppfs_ecc_extent& x : ext) {
            const size_t n = std::min<size_t>(x.length, ds - x.offset);
            static_vector<uint8_t> v(fresh.data() + x.pos, n, n);
            failed += !b->writeBlock(v, DataLocation((int)x.block, x.offset));
        }
        EXPECT_TRUE(std::memcmp(da.bytes(), db.bytes(), NB * raw) == 0);
        EXPECT_TRUE(same_log(*la, *lb));
        // off the disk, and the damage -- except for RS, which never fails a block: it logs what its decoder made of it
        EXPECT_TRUE(failed >= (rs || name == "raw255" ? 1u : 2u));
        EXPECT_TRUE(!corrects || lb->events.size() >= 1);
    }
}

int main()
{
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
    std::mt19937 rng(20241019);
    for (const auto& [name, make] : codecs) {
        for (const char* kind : { "stack", "plain" }) {
            g_case = std::string(name) + "/" + kind;
            Pair p;
            for (int k = 0; k < 2; ++k) {
                if (kind[0] == 's') {
                    auto d = std::make_unique<StackDisk<16>>();
                    p.bytes[k] = d->mapped();
                    p.disk[k] = std::move(d);
                } else {
                    auto d = std::make_unique<PlainDisk>(kDiskBytes);
                    p.bytes[k] = d->bytes();
                    p.disk[k] = std::move(d);
                }
                p.log[k] = std::make_shared<Logger>();
            }
            EXPECT_TRUE(p.bytes[0] && p.bytes[1]);
            if (!p.bytes[0] || !p.bytes[1])
                continue;
            for (int k = 0; k < 2; ++k)
                p.dev[k] = make(*p.disk[k], p.log[k]);
            run_extents(p, rng);
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
