// test_block_inode_write.cpp -- writeInodes of the C++ adapter (include/ppfs_gpu/block_device.hpp) on the GPU,
// differentially: one writeInodes call on one device is compared with IBlockDevice::writeInodes, the per-inode loop
// that is its definition (InodeManager::update: Bitmap::getBit, then _writeInode), on a second device over a copy of
// the disk -- per inode the result and the error, then the whole disk image and the correction log in order, and the inodes read
// back.  Variants: a clean disk, one error the code corrects in a bitmap block and in a table block that several
// inodes of the batch share, and a table block in mid-batch damaged beyond repair.  There the one call also writes
// the piece behind an inode's failing piece, which the loop does not reach: the block after the damaged one is
// compared through the inodes that both wrote, every other block byte for byte.
// Disks: StackDisk and MappedFileDisk (mapped: one engine call on the image) and a plain in-memory disk without a
// mapping (the per-inode loop).
//
// usage: test_block_inode_write <directory for the file-backed disks>
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

constexpr size_t kDiskBytes = (size_t)1 << 18; // StackDisk<18>

using MakeDevice = std::function<std::unique_ptr<IBlockDevice>(IDisk&, std::shared_ptr<Logger>)>;
using Table = IBlockDevice::InodeTable;
using Inode = IBlockDevice::PackedInode;

struct Pair { // the device under test and its twin, each on its own disk
    std::unique_ptr<IDisk> disk[2];
    uint8_t* bytes[2];
    std::shared_ptr<Logger> log[2];
    std::unique_ptr<IBlockDevice> dev[2];
};

// bytes at byte `at` of the payload stream that starts at block `first`, cut at block boundaries (_writeInode)
static void write_stream(IBlockDevice& d, uint32_t first, size_t at, const uint8_t* src, size_t n)
{
    const size_t ds = d.dataSize();
    while (n) {
        const size_t off = at % ds, len = std::min(n, ds - off);
        static_vector<uint8_t> v(const_cast<uint8_t*>(src), len, len);
        auto r = d.writeBlock(v, DataLocation((int)(first + at / ds), off));
        EXPECT_TRUE(r && *r == len);
        at += len, src += len, n -= len;
    }
}

struct Layout {
    Table table;
    std::vector<Inode> inodes;
    std::vector<bool> free;
};

static Layout build_table(Pair& p, std::mt19937& rng, uint32_t total)
{
    IBlockDevice& a = *p.dev[0];
    const size_t ds = a.dataSize();
    std::memset(p.bytes[0], 0, kDiskBytes);
    Layout L;
    const uint32_t bm_blocks = (uint32_t)(((total + 7) / 8 + ds - 1) / ds);
    L.table = Table { 1 + bm_blocks + 2, 1, total, 1 };
    EXPECT_TRUE(L.table.table_block + (81 * (size_t)total + ds - 1) / ds + 2 <= a.numOfBlocks());
    for (size_t b = 0; b < a.numOfBlocks() && b < L.table.table_block + (81 * (size_t)total + ds - 1) / ds + 2; ++b)
        EXPECT_TRUE((bool)a.formatBlock((block_index_t)b));
    L.inodes.resize(total);
    L.free.resize(total);
    std::vector<uint8_t> bitmap((total + 7) / 8, 0);
    for (uint32_t i = 0; i < total; ++i) {
        uint8_t* raw = reinterpret_cast<uint8_t*>(&L.inodes[i]);
        for (size_t k = 0; k < sizeof(Inode); ++k)
            raw[k] = (uint8_t)rng();
        L.free[i] = rng() % 4 == 0 && !(i + 4 >= total / 2 && i <= total / 2 + 4); // the damaged block's inodes stay allocated
        if (L.free[i])
            bitmap[i / 8] |= (uint8_t)(0x80 >> (i % 8));
        write_stream(a, L.table.table_block, sizeof(Inode) * (size_t)i, raw, sizeof(Inode));
    }
    write_stream(a, L.table.bitmap_block, 0, bitmap.data(), bitmap.size());
    return L;
}

static void run_batch(Pair& p, const Layout& L, const std::vector<uint32_t>& numbers, const std::vector<uint8_t>& start, int check,
    size_t failed_block, std::mt19937& rng)
{
    for (int k = 0; k < 2; ++k) {
        std::memcpy(p.bytes[k], start.data(), kDiskBytes);
        p.log[k]->events.clear();
    }
    Table t = L.table;
    t.check_bitmap = (uint32_t)check;
    const size_t n = numbers.size(), raw = p.dev[0]->rawBlockSize();
    std::vector<Inode> inodes(n);
    for (size_t j = 0; j < n; ++j) {
        uint8_t* bytes = reinterpret_cast<uint8_t*>(&inodes[j]);
        for (size_t k = 0; k < sizeof(Inode); ++k)
            bytes[k] = (uint8_t)rng();
    }
    std::vector<IBlockDevice::InodeWrite> got(n), want(n);
    std::memset((void*)got.data(), 0xCD, n * sizeof(got[0]));
    p.dev[0]->writeInodes(t, numbers.data(), n, inodes.data(), got.data());
    p.dev[1]->IBlockDevice::writeInodes(t, numbers.data(), n, inodes.data(), want.data()); // the per-inode loop
    size_t ok = 0, failed = 0, absent = 0, range = 0;
    for (size_t j = 0; j < n; ++j) {
        EXPECT_TRUE(got[j].ok == want[j].ok);
        EXPECT_TRUE(got[j].ok || got[j].error == want[j].error);
        ok += want[j].ok;
        failed += !want[j].ok && want[j].error == FsError::BlockDevice_CorrectionError;
        absent += !want[j].ok && want[j].error == FsError::InodeManager_NotFound;
        range += !want[j].ok && want[j].error == FsError::Bitmap_IndexOutOfRange;
    }
    EXPECT_TRUE(ok > 0 && range == 2 && (absent > 0) == (check != 0) && ok + failed + absent + range == n);
    if (failed_block)
        EXPECT_TRUE(failed > 0 && failed < n);
    EXPECT_TRUE(p.log[0]->events.size() == p.log[1]->events.size());
    for (size_t i = 0; i < std::min(p.log[0]->events.size(), p.log[1]->events.size()); ++i)
        EXPECT_TRUE(p.log[0]->events[i].block_index == p.log[1]->events[i].block_index);
    if (!failed_block) {
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    } else { // all but the block behind the failed one, where the one call wrote a straddler's second piece as well
        const size_t skip = (failed_block + 1) * raw;
        EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], skip) == 0);
        EXPECT_TRUE(std::memcmp(p.bytes[0] + skip + raw, p.bytes[1] + skip + raw, kDiskBytes - skip - raw) == 0);
        EXPECT_TRUE(std::memcmp(p.bytes[0] + failed_block * raw, start.data() + failed_block * raw, raw) == 0);
    }
    EXPECT_TRUE(std::memcmp(p.bytes[1], start.data(), kDiskBytes) != 0);
    // read back on both: every inode that was written holds its last record of the batch
    t.check_bitmap = 0;
    for (int k = 0; k < 2; ++k) {
        std::vector<IBlockDevice::InodeRead> back(n);
        p.dev[k]->IBlockDevice::readInodes(t, numbers.data(), n, back.data());
        for (size_t j = 0; j < n; ++j) {
            if (!want[j].ok)
                continue;
            size_t last = j;
            for (size_t q = j + 1; q < n; ++q)
                if (numbers[q] == numbers[j] && want[q].ok)
                    last = q;
            EXPECT_TRUE(back[j].ok && std::memcmp(&back[j].inode, &inodes[last], sizeof(Inode)) == 0);
        }
    }
}

// fixes: one error the code corrects in the bitmap's first block and in the table block that holds inode `at`'s
// first byte; fail: that table block damaged beyond repair instead
static void run_table(Pair& p, std::mt19937& rng, uint32_t total, bool fixes, bool fail, bool bit_errors)
{
    const Layout L = build_table(p, rng, total);
    IBlockDevice& a = *p.dev[0];
    const size_t raw = a.rawBlockSize(), ds = a.dataSize();
    const uint32_t at = total / 2;
    const size_t block = L.table.table_block + 81 * (size_t)at / ds;
    if (fixes) {
        p.bytes[0][(size_t)L.table.bitmap_block * raw + 1] ^= bit_errors ? 0x10 : 0x5A;
        p.bytes[0][block * raw + 2] ^= bit_errors ? 0x02 : 0xC3;
    }
    if (fail) {
        uint8_t* row = p.bytes[0] + block * raw; // two flipped bits: a CRC detects them, Hamming reports a double error
        row[3] ^= 0x01;
        row[raw / 2 + 1] ^= 0x10;
    }
    const std::vector<uint8_t> start(p.bytes[0], p.bytes[0] + kDiskBytes);
    std::vector<uint32_t> numbers;
    for (uint32_t i = at > 4 ? at - 4 : 0; i < at + 5 && i < total; ++i) // the neighbours that share the damaged block
        numbers.push_back(i);
    numbers.insert(numbers.end(), { total - 1, total, 0u, 0xFFFFFFFFu, at, 1u });
    for (int k = 0; k < 24; ++k)
        numbers.push_back((uint32_t)(rng() % total));
    run_batch(p, L, numbers, start, 1, fail ? block : 0, rng);
    run_batch(p, L, numbers, start, 0, fail ? block : 0, rng);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    struct Codec {
        const char* name;
        MakeDevice make;
        uint32_t total;
        bool corrects, bit_errors; // an error is corrected and logged; it has to be a single bit
        bool can_fail;             // a block of noise is reported as beyond the code's capability
    };
    const std::vector<Codec> codecs = {
        { "rs255t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 255, 3, l); }, 300, true,
            false, false },
        { "rs64t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 64, 3, l); }, 300, true, false,
            false },
        { "crc64",
            [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<CrcBlockDevice>(CrcPolynomial::MsgImplicit(0x9960034c), d, 64, l); },
            300, false, false, true },
        { "hamming256", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<HammingBlockDevice>(8, d, l); }, 300, true, true, true },
        { "parity32", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ParityBlockDevice>(32, d, l); }, 300, false, false,
            false },
    };
    std::mt19937 rng(20250404);
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
            run_table(p, rng, c.total, false, false, false);
            if (c.corrects) {
                g_case += "/corrected";
                run_table(p, rng, c.total, true, false, c.bit_errors);
                EXPECT_TRUE(p.log[1]->events.size() >= 1);
            }
            if (c.can_fail) {
                g_case = std::string(c.name) + "/" + kind + "/failing";
                run_table(p, rng, c.total, false, true, false); // an inode in mid-batch damaged beyond repair
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
