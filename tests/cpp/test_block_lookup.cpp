// test_block_lookup.cpp -- lookupNames / lookupInodes of the C++ adapter (include/ppfs_gpu/block_device.hpp) on the
// GPU, differentially: one call on one device is compared with IBlockDevice::lookup_loop, the loop of
// DirectoryManager::getInodeByName (and of removeEntry's search) that is its definition, on a second device over a copy
// of the disk -- per query the result, the error, the inode and the entry, then the adapter contract for the disk and
// the correction log: the loop's events first and in the loop's order; behind them the blocks that the engine, which
// reads every directory whole, corrected beyond the loop's reach; the disk the loop's with exactly those blocks
// corrected as well.  Three directories (no entry, five, many) are written through the adapter the way the reference
// writes them: index blocks as entries at {block, 0} of a formatted block, data blocks as writes of their bytes.
// Variants: a clean disk; one error the code corrects in the indirect block and one in a data block of the second
// batch; a data block of the first batch damaged beyond repair with a correctable block in the second batch, which no
// readFile of any loop touches.
// Disks: StackDisk and MappedFileDisk (mapped: one engine call on the image) and a plain in-memory disk without a
// mapping (the loop).
//
// usage: test_block_lookup <directory for the file-backed disks>
// Exit status 0 and "ALL PASSED" on success.  Needs a GPU (the adapter has no CPU fallback).
#include "ppfs_gpu/block_device.hpp"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <memory>
#include <random>
#include <set>
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
using Lookup = IBlockDevice::Lookup;

struct Pair { // the device under test and its twin, each on its own disk
    std::unique_ptr<IDisk> disk[2];
    uint8_t* bytes[2];
    std::shared_ptr<Logger> log[2];
    std::unique_ptr<IBlockDevice> dev[2];
};

struct Dirs {
    std::vector<ppfs_ecc_file> files;                   // no entry, five entries, `many` entries
    std::vector<std::vector<std::string>> names;        // per directory, per entry
    std::vector<std::vector<block_index_t>> data_block; // per directory, per file block
    block_index_t indirect_of_last = 0;
};

// A file of `bytes` bytes whose payload is `payload`: data blocks from `next` on, then its index blocks
static ppfs_ecc_file build_file(IBlockDevice& d, block_index_t& next, const std::vector<uint8_t>& payload, size_t file_size,
    std::vector<block_index_t>& data_block, block_index_t* indirect)
{
    const size_t ds = d.dataSize(), ipb = ds / 4, nblocks = (file_size + ds - 1) / ds;
    ppfs_ecc_file f {};
    f.file_size = (uint32_t)file_size;
    data_block.clear();
    for (size_t j = 0; j < nblocks; ++j) {
        const block_index_t b = next++;
        data_block.push_back(b);
        EXPECT_TRUE((bool)d.formatBlock(b));
        const size_t at = j * ds, len = std::min(ds, payload.size() > at ? payload.size() - at : 0);
        if (len) {
            static_vector<uint8_t> v(const_cast<uint8_t*>(payload.data() + at), len, len);
            auto r = d.writeBlock(v, DataLocation((int)b, 0));
            EXPECT_TRUE(r && *r == len);
        }
    }
    auto index_block = [&](const std::vector<block_index_t>& entries) {
        const block_index_t b = next++;
        EXPECT_TRUE((bool)d.formatBlock(b));
        static_vector<uint8_t> v(reinterpret_cast<uint8_t*>(const_cast<block_index_t*>(entries.data())), 4 * entries.size(), 4 * entries.size());
        auto r = d.writeBlock(v, DataLocation((int)b, 0));
        EXPECT_TRUE(r && *r == 4 * entries.size());
        return b;
    };
    for (size_t j = 0; j < nblocks && j < 12; ++j)
        f.direct[j] = data_block[j];
    if (nblocks > 12) {
        std::vector<block_index_t> e(data_block.begin() + 12, data_block.begin() + std::min(nblocks, 12 + ipb));
        f.indirect = index_block(e);
        if (indirect)
            *indirect = f.indirect;
    }
    if (nblocks > 12 + ipb) {
        std::vector<block_index_t> leaves;
        for (size_t at = 12 + ipb; at < nblocks; at += ipb)
            leaves.push_back(index_block(std::vector<block_index_t>(data_block.begin() + at, data_block.begin() + std::min(nblocks, at + ipb))));
        EXPECT_TRUE(leaves.size() <= ipb);
        f.doubly_indirect = index_block(leaves);
    }
    return f;
}

static Dirs build_dirs(Pair& p, size_t many)
{
    IBlockDevice& a = *p.dev[0];
    std::memset(p.bytes[0], 0, kDiskBytes);
    Dirs D;
    block_index_t next = 3;
    const size_t counts[3] = { 0, 5, many }, trailing[3] = { 100, 0, 77 };
    for (int d = 0; d < 3; ++d) {
        std::vector<std::string> names;
        std::vector<uint8_t> payload(counts[d] * 128, 0xEE); // garbage behind every NUL
        for (size_t i = 0; i < counts[d]; ++i) {
            std::string nm = i % 3 ? "common_prefix_" + std::to_string(d) + "_" + std::to_string(1000 + i) : "e" + std::to_string(i);
            if (d == 2 && (i == 10 || i == many - 20))
                nm = "twice"; // the first wins
            if (d == 2 && i == many - 9)
                nm = "";
            if (d == 2 && i == many - 7)
                nm = std::string(123, 'L');
            names.push_back(nm);
            uint8_t* e = payload.data() + 128 * i;
            const uint32_t inode = 7000u * (uint32_t)(d + 1) + (uint32_t)i;
            std::memcpy(e, &inode, 4);
            std::memcpy(e + 4, nm.data(), nm.size());
            e[4 + nm.size()] = 0;
        }
        if (d == 2)
            std::memset(payload.data() + 128 * 50 + 4, 'U', 124); // an unterminated entry: matches nothing
        std::vector<block_index_t> blocks;
        D.files.push_back(build_file(a, next, payload, counts[d] * 128 + trailing[d], blocks, d == 2 ? &D.indirect_of_last : nullptr));
        D.names.push_back(names);
        D.data_block.push_back(blocks);
    }
    EXPECT_TRUE((size_t)next + 2 <= a.numOfBlocks());
    return D;
}

struct Queries {
    std::vector<std::vector<uint8_t>> records; // the 128-byte name records
    std::vector<Lookup> by_name, by_inode;
};
static Queries make_queries(const Dirs& D, size_t many)
{
    Queries Q;
    auto name = [&](uint32_t dir, const std::string& s, bool terminated = true) {
        std::vector<uint8_t> rec(128, 0xC3); // garbage behind the query's NUL
        std::memcpy(rec.data(), s.data(), std::min<size_t>(s.size(), 128));
        if (terminated && s.size() < 128)
            rec[s.size()] = 0;
        Q.records.push_back(rec);
        Q.by_name.push_back(Lookup { dir, 0xABCDu, nullptr, true, FsError {}, 1, 1 });
    };
    const auto& nm = D.names[2];
    for (size_t i : { (size_t)0, (size_t)1, many - 1, many / 2, (size_t)10, many - 20, many - 9, many - 7, many - 2, (size_t)0, many - 1 })
        name(2, nm[i]);
    name(2, "nope");
    name(2, nm[1].substr(0, nm[1].size() - 1));
    name(2, nm[1] + "0");
    name(2, std::string(123, 'U'));
    name(2, std::string(124, 'U'));
    name(2, std::string(128, 'U'), false);
    name(2, std::string(122, 'L'));
    for (size_t i : { (size_t)0, (size_t)4, (size_t)2 })
        name(1, D.names[1][i]);
    name(1, "nope");
    name(1, nm[0]);
    name(0, "anything");
    name(0, "");
    for (size_t q = 0; q < Q.by_name.size(); ++q)
        Q.by_name[q].name = Q.records[q].data();
    auto key = [&](uint32_t dir, uint32_t k) { Q.by_inode.push_back(Lookup { dir, k, nullptr, true, FsError {}, 1, 1 }); };
    for (uint32_t k : { 21000u, 21000u + (uint32_t)many - 1, 21011u, 21000u + (uint32_t)many / 2, 5u, 21000u + (uint32_t)many, 21000u + (uint32_t)many - 1 })
        key(2, k);
    for (uint32_t k : { 14000u, 14004u, 14005u })
        key(1, k);
    key(0, 7000u);
    return Q;
}

// returns the number of blocks the device under test corrected beyond the loop's reach
static size_t run_lookup(Pair& p, const Dirs& D, const Queries& Q, const std::vector<uint8_t>& start, bool by_name, bool mapped, int want_failed)
{
    for (int k = 0; k < 2; ++k) {
        std::memcpy(p.bytes[k], start.data(), kDiskBytes);
        p.log[k]->events.clear();
    }
    std::vector<Lookup> got = by_name ? Q.by_name : Q.by_inode, want = got;
    if (by_name) {
        p.dev[0]->lookupNames(D.files.data(), D.files.size(), got.data(), got.size());
    } else {
        p.dev[0]->lookupInodes(D.files.data(), D.files.size(), got.data(), got.size());
    }
    p.dev[1]->IBlockDevice::lookup_loop(D.files.data(), D.files.size(), want.data(), want.size(), by_name); // the loop
    size_t found = 0, absent = 0, failed = 0;
    for (size_t q = 0; q < got.size(); ++q) {
        EXPECT_TRUE(got[q].ok == want[q].ok && got[q].inode == want[q].inode && got[q].entry == want[q].entry);
        EXPECT_TRUE(got[q].ok || got[q].error == want[q].error);
        EXPECT_TRUE(want[q].ok == (want[q].inode != 0xFFFFFFFFu) && want[q].ok == (want[q].entry != 0xFFFFFFFFu));
        found += want[q].ok;
        absent += !want[q].ok && want[q].error == (by_name ? FsError::PpFS_NotFound : FsError::DirectoryManager_NotFound);
        failed += !want[q].ok && want[q].error == FsError::BlockDevice_CorrectionError;
    }
    EXPECT_TRUE(found >= 2 && absent >= 2 && found + absent + failed == got.size());
    EXPECT_TRUE(want_failed < 0 || (want_failed ? failed > 0 : failed == 0));
    // the log: the loop's events first and in order, then the blocks corrected beyond the loop's reach, each once
    const auto &mine = p.log[0]->events, &theirs = p.log[1]->events;
    EXPECT_TRUE(mine.size() >= theirs.size());
    for (size_t i = 0; i < std::min(mine.size(), theirs.size()); ++i)
        EXPECT_TRUE(mine[i].block_index == theirs[i].block_index);
    std::set<size_t> extra;
    for (size_t i = theirs.size(); i < mine.size(); ++i)
        EXPECT_TRUE(extra.insert((size_t)mine[i].block_index).second);
    EXPECT_TRUE(mapped || extra.empty());
    // the disk: the loop's, with exactly those blocks corrected as well
    const size_t raw = p.dev[0]->rawBlockSize();
    std::set<size_t> differ;
    for (size_t b = 0; b < kDiskBytes / raw; ++b)
        if (std::memcmp(p.bytes[0] + b * raw, p.bytes[1] + b * raw, raw) != 0)
            differ.insert(b);
    EXPECT_TRUE(differ == extra);
    for (size_t b : extra) { // corrected: the twin's own read of the block repairs it to the same bytes
        std::vector<uint8_t> one(1);
        static_vector<uint8_t> v(one.data(), 1, 0);
        EXPECT_TRUE((bool)p.dev[1]->readBlock(DataLocation((int)b, 0), 1, v));
    }
    EXPECT_TRUE(std::memcmp(p.bytes[0], p.bytes[1], kDiskBytes) == 0);
    return extra.size();
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    struct Codec {
        const char* name;
        MakeDevice make;
        size_t many;
        bool corrects, bit_errors; // an error is corrected and logged; it has to be a single bit
        bool can_fail;             // two flipped bits are reported as beyond the code's capability
    };
    const std::vector<Codec> codecs = {
        { "rs255t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 255, 3, l); }, 300, true,
            false, false },
        // ds = 58, 14 pointers a block: 90 entries stay within the doubly indirect tree (one batch; the code keeps the loop)
        { "rs64t3", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ReedSolomonBlockDevice>(d, 64, 3, l); }, 90, true, false,
            false },
        { "crc256",
            [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<CrcBlockDevice>(CrcPolynomial::MsgImplicit(0x9960034c), d, 256, l); },
            300, false, false, true },
        { "hamming256", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<HammingBlockDevice>(8, d, l); }, 300, true, true, true },
        { "parity128", [](IDisk& d, std::shared_ptr<Logger> l) { return std::make_unique<ParityBlockDevice>(128, d, l); }, 300, false, false,
            false },
    };
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
            const bool mapped = kind[0] != 'p';
            const Dirs D = build_dirs(p, c.many);
            const Queries Q = make_queries(D, c.many);
            const std::vector<uint8_t> clean(p.bytes[0], p.bytes[0] + kDiskBytes);
            const size_t raw = p.dev[0]->rawBlockSize(), ds = p.dev[0]->dataSize();
            const auto& blocks = D.data_block[2];
            const size_t early = (128 * 40) / ds, late = (128 * (c.many - 10)) / ds; // under entry 40; under one of the last entries
            for (bool by_name : { true, false }) {
                run_lookup(p, D, Q, clean, by_name, mapped, 0);
                EXPECT_TRUE(p.log[0]->events.empty());
                if (c.corrects) {
                    g_case = std::string(c.name) + "/" + kind + "/corrected";
                    std::vector<uint8_t> image = clean;
                    if (D.indirect_of_last)
                        image[(size_t)D.indirect_of_last * raw + 2] ^= c.bit_errors ? 0x02 : 0xC3;
                    image[(size_t)blocks[late] * raw + 1] ^= c.bit_errors ? 0x10 : 0x5A;
                    run_lookup(p, D, Q, image, by_name, mapped, 0);
                    EXPECT_TRUE(p.log[1]->events.size() >= 2);
                }
                if (c.can_fail) {
                    g_case = std::string(c.name) + "/" + kind + "/failing";
                    std::vector<uint8_t> image = clean;
                    uint8_t* row = image.data() + (size_t)blocks[early] * raw; // two flipped bits: every loop over the directory ends here
                    row[3] ^= 0x01;
                    row[raw / 2 + 1] ^= 0x10;
                    const bool beyond = c.corrects && c.many > 256 && late > (256 * 128 - 1) / ds; // a block of the second batch
                    if (beyond) // no loop reaches it, the engine corrects it
                        image[(size_t)blocks[late] * raw + 1] ^= 0x10;
                    const size_t extra = run_lookup(p, D, Q, image, by_name, mapped, 1);
                    EXPECT_TRUE(extra == (beyond && mapped ? 1u : 0u));
                }
                g_case = std::string(c.name) + "/" + kind;
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
