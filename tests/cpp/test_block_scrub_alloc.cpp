// test_block_scrub_alloc.cpp -- scrubList / scrubAllocated of the C++ adapter
// (include/ppfs_gpu/block_device.hpp) on the GPU, differentially: each call on one device is compared
// with the per-block readBlock loop over the same blocks on a second device over a copy of the disk --
// per-block errors (255 for a block whose bit is clear), the bitmap blocks' errors, the whole disk image,
// the correction log in order, and the counts.  The bitmap is written the way the reference's
// Bitmap::setBit writes it: one byte at {bitmap_block + byte / dataSize(), byte % dataSize()}.
// Disks: StackDisk and MappedFileDisk (mapped: one engine call on the image) and a plain in-memory disk
// without a mapping (the per-block loop).
//
// usage: test_block_scrub_alloc <directory for the file-backed disks>
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

constexpr size_t kDiskBytes = (size_t)1 << 16; // StackDisk<16>
constexpr block_index_t kBitmapBlock = 2;

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

// readBlock({blk, 0}, dataSize()) on the twin: its FsError (0: none), the payload in `one`
static uint8_t read_one(IBlockDevice& b, block_index_t blk, std::vector<uint8_t>& one)
{
    static_vector<uint8_t> v(one.data(), one.size(), 0);
    auto r = b.readBlock(DataLocation((int)blk, 0), one.size(), v);
    return r ? 0 : (uint8_t)r.error();
}

static void run_allocated(Pair& p, std::mt19937& rng, size_t nbits, unsigned bitmap_flips)
{
    IBlockDevice& a = *p.dev[0];
    IBlockDevice& b = *p.dev[1];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize(), B = a.bitmapBlocks(nbits);
    const block_index_t first = kBitmapBlock + (block_index_t)B + 1;
    const size_t on_disk = std::min<size_t>(a.numOfBlocks(), first + nbits);
    EXPECT_TRUE(raw > 0 && ds > 0 && first < a.numOfBlocks());
    if (!raw || !ds || first >= a.numOfBlocks())
        return;
    // a written disk, the bitmap set bit by bit, damage of every weight the codec meets
    std::memset(p.bytes[0], 0, kDiskBytes);
    std::vector<uint8_t> payloads(on_disk * ds, 0), err(std::max(on_disk, nbits));
    for (size_t i = (size_t)first * ds; i < payloads.size(); ++i)
        payloads[i] = (uint8_t)rng();
    EXPECT_TRUE((bool)a.writeBlocks(0, on_disk, payloads.data(), err.data()));
    std::vector<uint8_t> bits(nbits);
    for (size_t j = 0; j < nbits; ++j)
        bits[j] = j + 1 == nbits || rng() % 3 == 0;
    for (size_t byte = 0; byte < (nbits + 7) / 8; ++byte) {
        uint8_t v = 0;
        for (size_t k = 0; k < 8 && 8 * byte + k < nbits; ++k)
            v |= bits[8 * byte + k] ? (uint8_t)(0x80u >> k) : 0;
        static_vector<uint8_t> one(&v, 1, 1);
        EXPECT_TRUE((bool)a.writeBlock(one, DataLocation((int)(kBitmapBlock + byte / ds), (int)(byte % ds))));
    }
    for (size_t blk = first; blk < on_disk; blk += 2)
        for (size_t k = 0; k < 1 + blk % 3; ++k)
            p.bytes[0][blk * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    for (unsigned k = 0; k < bitmap_flips; ++k) // in the bitmap's last block
        p.bytes[0][(kBitmapBlock + B - 1) * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    std::memcpy(p.bytes[1], p.bytes[0], kDiskBytes);
    p.log[0]->events.clear();
    p.log[1]->events.clear();

    std::vector<uint8_t> e(nbits, 0xEE), be(B, 0xEE), one(ds);
    ppfs_ecc_scrub_counts c;
    std::memset(&c, 0xEE, sizeof c);
    EXPECT_TRUE((bool)a.scrubAllocated(kBitmapBlock, first, nbits, &c, e.data(), be.data()));

    // the per-block loop: the bitmap's blocks, then the allocated blocks in ascending order
    ppfs_ecc_scrub_counts w {};
    std::vector<uint8_t> stream(B * ds, 0), bfail(B, 0);
    for (size_t k = 0; k < B; ++k) {
        const size_t before = p.log[1]->events.size();
        bfail[k] = read_one(b, kBitmapBlock + (block_index_t)k, one);
        EXPECT_TRUE(be[k] == bfail[k]);
        std::memcpy(stream.data() + k * ds, one.data(), ds);
        ++(bfail[k] ? w.bitmap_failed : p.log[1]->events.size() > before ? w.bitmap_corrected : w.bitmap_ok);
    }
    for (size_t j = 0; j < nbits; ++j) {
        const bool set = bfail[j / (8 * ds)] || (stream[j / 8] & (0x80u >> (j % 8)));
        if (!set) {
            EXPECT_TRUE(e[j] == PPFS_ECC_NOT_ALLOCATED);
            ++w.not_allocated;
            continue;
        }
        const size_t before = p.log[1]->events.size();
        const uint8_t x = read_one(b, first + (block_index_t)j, one);
        EXPECT_TRUE(e[j] == x);
        ++(x == (uint8_t)FsError::Disk_OutOfBounds ? w.out_of_range
                : x                                ? w.failed
                : p.log[1]->events.size() > before ? w.corrected
                                                   : w.ok);
    }
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));
    EXPECT_TRUE(std::memcmp(&c, &w, sizeof c) == 0);
    EXPECT_TRUE(w.not_allocated < nbits && (bitmap_flips || w.not_allocated > 0)); // a failed bitmap block sets its bits
}

static void run_list(Pair& p, std::mt19937& rng)
{
    IBlockDevice& a = *p.dev[0];
    IBlockDevice& b = *p.dev[1];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize(), nb = 96;
    std::vector<uint8_t> payloads(nb * ds), err(nb);
    for (auto& x : payloads)
        x = (uint8_t)rng();
    EXPECT_TRUE((bool)a.writeBlocks(0, nb, payloads.data(), err.data()));
    for (size_t blk = 0; blk < nb; blk += 3)
        for (size_t k = 0; k < 1 + blk % 3; ++k)
            p.bytes[0][blk * raw + rng() % raw] ^= (uint8_t)(1u << (rng() % 8));
    std::memcpy(p.bytes[1], p.bytes[0], kDiskBytes);
    p.log[0]->events.clear();
    p.log[1]->events.clear();
    std::vector<block_index_t> ix;
    for (block_index_t i = 0; i < nb; i += 2)
        ix.push_back(i);
    std::shuffle(ix.begin(), ix.end(), rng);
    ix.insert(ix.begin() + 5, { (block_index_t)a.numOfBlocks(), (block_index_t)a.numOfBlocks() + 7 }); // off the disk
    ix.push_back(ix[1]);                                                                              // a repeat
    std::vector<uint8_t> e(ix.size(), 0xEE), one(ds);
    ppfs_ecc_scrub_counts c, w {};
    std::memset(&c, 0xEE, sizeof c);
    EXPECT_TRUE((bool)a.scrubList(ix.data(), ix.size(), &c, e.data()));
    for (size_t k = 0; k < ix.size(); ++k) {
        const size_t before = p.log[1]->events.size();
        const uint8_t x = read_one(b, ix[k], one);
        EXPECT_TRUE(e[k] == x);
        ++(x == (uint8_t)FsError::Disk_OutOfBounds ? w.out_of_range
                : x                                ? w.failed
                : p.log[1]->events.size() > before ? w.corrected
                                                   : w.ok);
    }
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    EXPECT_TRUE(same_log(*p.log[0], *p.log[1]));
    EXPECT_TRUE(std::memcmp(&c, &w, sizeof c) == 0);
}

static void run_lists(Pair& p, std::mt19937& rng)
{
    run_list(p, rng);
    run_allocated(p, rng, 150, 0);
    run_allocated(p, rng, 150, 1); // a damaged bitmap block: corrected (RS, Hamming) or failed, all its bits set
    run_allocated(p, rng, 150, 2);
    if (p.dev[0]->numOfBlocks() <= 1100) { // the bit range runs three blocks past the disk
        const size_t n = p.dev[0]->numOfBlocks() - kBitmapBlock - 1;
        run_allocated(p, rng, n - p.dev[0]->bitmapBlocks(n) + 3, 0);
    }
}

// scrubList / scrubAllocated with counts, err and bitmap_err null == the per-block loop: the disk image and
// the log in order.  The disk is 8 blocks, mapped or not: the bitmap in block 0, blocks 1..7 its bits, one
// allocated block with a single flipped bit and one damaged past what the codec corrects; the list adds an
// index past the disk and a repeated one, so the calls meet ok, corrected, failed, out of bounds and not
// allocated with nowhere to report them.
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
        std::vector<uint8_t> payloads(NB * ds, 0), err(NB), one(ds);
        for (size_t i = ds; i < payloads.size(); ++i)
            payloads[i] = (uint8_t)rng();
        payloads[0] = 0xDA; // bits 0, 1, 3, 4 and 6 set: blocks 1, 2, 4, 5 and 7 are allocated
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

        damaged();
        const std::vector<block_index_t> ix = { 4, 2, (block_index_t)a->numOfBlocks(), 5, 2, 0 };
        EXPECT_TRUE((bool)a->scrubList(ix.data(), ix.size(), nullptr, nullptr));
        size_t failed = 0;
        for (block_index_t blk : ix)
            failed += read_one(*b, blk, one) != 0;
        EXPECT_TRUE(std::memcmp(da.bytes(), db.bytes(), NB * raw) == 0);
        EXPECT_TRUE(same_log(*la, *lb));
        // off the disk, and the damage -- except for RS, which never fails a block: it logs what its decoder made of it
        EXPECT_TRUE(failed >= (rs || name == "raw255" ? 1u : 2u));
        EXPECT_TRUE(!corrects || lb->events.size() >= 1);

        damaged();
        EXPECT_TRUE((bool)a->scrubAllocated(0, 1, NB - 1, nullptr, nullptr, nullptr));
        EXPECT_TRUE(read_one(*b, 0, one) == 0 && one[0] == 0xDA); // the bitmap's block, then its set bits' blocks
        for (block_index_t blk : { 1, 2, 4, 5, 7 })
            (void)read_one(*b, blk, one);
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
