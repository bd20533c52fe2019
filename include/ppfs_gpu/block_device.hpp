#pragma once
/*
 * ppfs_gpu/block_device.hpp -- C++17 host mirror of PPFS's block-device layer, backed by the
 * MI355X ECC engine (include/ppfs_ecc.h).  Header-only; link with libppfs_ecc.so.
 *
 * Same class names, constructor arguments, return conventions and error behaviour as the
 * reference, so PPFS code (FileIO, Bitmap, InodeManager, bench_blockdevice) can hold these
 * objects where it holds the reference's:
 *
 *   IBlockDevice               lib/blockdevice/include/ppfs/blockdevice/iblock_device.hpp:34-97
 *   DataLocation               iblock_device.hpp:14-20
 *   ReedSolomonBlockDevice     rs_block_device.hpp:20-80,  src/rs_block_device.cpp:9-93
 *   CrcBlockDevice             crc_block_device.hpp,       src/crc_block_device.cpp:12-134
 *   HammingBlockDevice         hamming_block_device.hpp,   src/hamming_block_device.cpp:11-172
 *   ParityBlockDevice          parity_block_device.hpp,    src/parity_block_device.cpp:9-97
 *   RawBlockDevice             raw_block_device.hpp,       src/raw_block_device.cpp
 *   CrcPolynomial              lib/ecc_helpers/include/ppfs/ecc_helpers/crc_polynomial.hpp
 *   IDisk / StackDisk          lib/disk/include/ppfs/disk/idisk.hpp:9-19, stack_disk.hpp:9-44
 *   static_vector              lib/common/include/ppfs/common/static_vector.hpp:11-100
 *   FsError                    lib/common/include/ppfs/common/types.hpp:11-80 (same order/values)
 *
 * The reference is C++23 (std::expected); this image's libstdc++ has no <expected>, so
 * ppfs_gpu::expected / unexpected carry the same interface (has_value, value, error,
 * operator bool).  Inside PPFS proper, alias them to std:: and drop the copies here.
 *
 * All codec arithmetic (RS encode / syndromes / Berlekamp-Massey / Chien / Forney, CRC,
 * Hamming SECDED, parity) runs in the HIP kernels behind the C ABI.  This layer moves bytes
 * between the disk and the engine and reproduces the reference's read-modify-write,
 * write-back and logging order.  There is no CPU fallback: every engine error (including a
 * device whose engine could not be created: no GPU, bad parameters) is reported as
 * FsError::Disk_IOError, with the ABI's message on stderr; nothing throws or aborts.
 *
 * Extension: readBlocks / writeBlocks run a contiguous range of whole blocks
 * through ONE engine call; results, disk contents and log are those of the per-block loop.
 * readBlockList / writeBlockList do the same for a list of block indices in any order (the blocks
 * of a fragmented file, as FileIO's BlockIndexIterator yields them).
 * readExtents / writeExtents take byte ranges (block, offset, length) of such blocks -- a file range
 * that starts and ends mid-block (file_extents), or a few bytes of an inode or bitmap block -- again
 * in one engine call.
 * fileBlocks / readFile take the 64 bytes of an inode that describe its index-block tree (ppfs_ecc_file)
 * and resolve the tree themselves: FileIO::readFile of any size without the BlockIndexIterator loop.
 * readFiles does that for a batch of (inode, offset, length) -- a directory scan, a backup -- with all the
 * files' trees walked in one engine call.
 * writeFile / writeFiles are the in-place case of FileIO::writeFile from the same 64 bytes: a range inside the
 * file, or a batch of them, written without the iterator loop; nothing is allocated and no inode is updated.
 *
 * Every one of those overrides in EngineBlockDevice is built from the same few steps, each of which exists once:
 * _wb (the engine calls' write_back flag), engine_image() (the mapped image, or null, for a batch engine call),
 * status_error() / report() (engine statuses as per-entry FsError bytes, correction events and zeroed payloads),
 * list_unmapped() (the list calls on a disk without a mapping), FileBatch (the file calls' selection, plan and
 * tree walk, and each file's events and first failing block) and inode_ok() / inode_log() (an inode call's statuses
 * as the loop's results, and its correction log from piece_status, for readInodes and writeInodes).  The comment above each override states its one
 * deviation from the per-block loop, which defines it.
 */
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <utility>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "ppfs_ecc.h"

#define MAX_BLOCK_SIZE 4096
#define MAX_RS_BLOCK_SIZE 255

namespace ppfs_gpu {

typedef std::uint32_t block_index_t;

enum class FsError : uint8_t {
    Bitmap_IndexOutOfRange,
    Bitmap_NotFound,
    BlockManager_AlreadyTaken,
    BlockManager_AlreadyFree,
    BlockManager_NoMoreFreeBlocks,
    BlockDevice_CorrectionError, // = 5
    DirectoryManager_NameTaken,
    DirectoryManager_NotFound,
    DirectoryManager_InvalidRequest,
    Disk_OutOfBounds, // = 9
    Disk_InvalidRequest, // = 10
    Disk_IOError, // = 11
    FileIO_OutOfBounds,
    FileIO_InternalError,
    FileIO_InvalidRequest,
    PpFS_DiskNotFormatted,
    PpFS_InvalidRequest,
    PpFS_NotInitialized,
    PpFS_InvalidPath,
    PpFS_NotFound,
    PpFS_FileInUse,
    PpFS_DirectoryNotEmpty,
    PpFS_OutOfBounds,
    PpFS_OpenFilesTableFull,
    PpFS_AlreadyOpen,
    InodeManager_AlreadyTaken,
    InodeManager_NotFound,
    InodeManager_AlreadyFree,
    InodeManager_NoMoreFreeInodes,
    Mutex_InitFailed,
    Mutex_LockFailed,
    Mutex_UnlockFailed,
    Mutex_NotInitialized,
    Mutex_AlreadyInitialized,
    Mutex_InternalError,
    SuperBlockManager_InvalidRequest,
    StaticVector_AllocationError,
    NotImplemented,
    Config_IOError,
    Config_SyntaxError,
    Config_InvalidValue,
    Config_MissingField,
    Config_UnknownKey
};
static_assert((int)FsError::BlockDevice_CorrectionError == PPFS_ECC_CORRECTION_ERROR, "status 5");
static_assert((int)FsError::Disk_OutOfBounds == PPFS_ECC_OUT_OF_BOUNDS, "status 9");
// a lookup's "ran to the end without a match" is no FsError of a block: the adapter turns it into PpFS_NotFound /
// DirectoryManager_NotFound, and it collides with no status a block can have
static_assert(PPFS_ECC_NOT_FOUND == 2 && PPFS_ECC_NOT_FOUND != PPFS_ECC_CORRECTED && PPFS_ECC_NOT_FOUND != PPFS_ECC_CORRECTION_ERROR
        && PPFS_ECC_NOT_FOUND != PPFS_ECC_OUT_OF_BOUNDS && PPFS_ECC_NOT_FOUND != PPFS_ECC_NOT_ALLOCATED && PPFS_ECC_NOT_FOUND != 0,
    "status 2: not found");

// ------------------------------------------------------------------------------------------
// std::expected<T, E> subset
// ------------------------------------------------------------------------------------------
template <class E> struct unexpected_t {
    E e;
};
template <class E> unexpected_t<E> unexpected(E e) { return { e }; }

template <class T, class E = FsError> class expected {
public:
    expected(T v)
        : _ok(true)
        , _v(std::move(v))
    {
    }
    expected(unexpected_t<E> u)
        : _ok(false)
        , _e(u.e)
    {
    }
    bool has_value() const { return _ok; }
    explicit operator bool() const { return _ok; }
    const T& value() const
    {
        if (!_ok) {
            std::fprintf(stderr, "ppfs_gpu::expected: bad access (error %d)\n", (int)_e);
            std::abort();
        }
        return _v;
    }
    const T& operator*() const { return _v; }
    E error() const { return _e; }

private:
    bool _ok;
    T _v {};
    E _e {};
};

template <class E> class expected<void, E> {
public:
    expected()
        : _ok(true)
    {
    }
    expected(unexpected_t<E> u)
        : _ok(false)
        , _e(u.e)
    {
    }
    bool has_value() const { return _ok; }
    explicit operator bool() const { return _ok; }
    void value() const
    {
        if (!_ok) {
            std::fprintf(stderr, "ppfs_gpu::expected: bad access (error %d)\n", (int)_e);
            std::abort();
        }
    }
    E error() const { return _e; }

private:
    bool _ok;
    E _e {};
};

// ------------------------------------------------------------------------------------------
// static_vector: non-owning view with a capacity (static_vector.hpp semantics)
// ------------------------------------------------------------------------------------------
template <typename T> class static_vector {
    static_assert(std::is_trivially_copyable<T>::value, "static_vector supports only trivially copyable types");

public:
    static_vector() = default;
    static_vector(T* buffer, std::size_t capacity, std::size_t size = 0)
        : _buffer(buffer)
        , _capacity(capacity)
        , _size(std::min(size, capacity))
    {
    }
    expected<void> push_back(const T& v)
    {
        if (_size >= _capacity)
            return unexpected(FsError::StaticVector_AllocationError);
        _buffer[_size++] = v;
        return {};
    }
    T& operator[](std::size_t i) { return _buffer[i]; }
    const T& operator[](std::size_t i) const { return _buffer[i]; }
    std::size_t size() const { return _size; }
    std::size_t capacity() const { return _capacity; }
    bool empty() const { return _size == 0; }
    T* begin() { return _buffer; }
    T* end() { return _buffer + _size; }
    const T* begin() const { return _buffer; }
    const T* end() const { return _buffer + _size; }
    T* data() { return _buffer; }
    const T* data() const { return _buffer; }
    expected<void> resize(std::size_t n)
    {
        if (n > _capacity)
            return unexpected(FsError::StaticVector_AllocationError);
        _size = n;
        return {};
    }
    expected<void> assign(std::initializer_list<T> init)
    {
        if (init.size() > _capacity)
            return unexpected(FsError::StaticVector_AllocationError);
        std::memcpy(_buffer, init.begin(), init.size() * sizeof(T));
        _size = init.size();
        return {};
    }

private:
    T* _buffer = nullptr;
    std::size_t _capacity = 0;
    std::size_t _size = 0;
};

struct DataLocation {
    int block_index = 0;
    size_t offset = 0;
    DataLocation(int b, size_t o)
        : block_index(b)
        , offset(o)
    {
    }
    DataLocation() = default;
};

// ------------------------------------------------------------------------------------------
// Disks
// ------------------------------------------------------------------------------------------
struct IDisk {
    virtual ~IDisk() = default;
    virtual expected<void> read(size_t address, size_t size, static_vector<uint8_t>& data) = 0;
    virtual expected<size_t> write(size_t address, const static_vector<uint8_t>& data) = 0;
    virtual size_t size() = 0;
    // Extension: a disk whose whole image is addressable host memory (size() bytes, writes
    // through it are the disk's writes).  The batch calls of the engine devices then run the
    // engine on the image in place -- no copy into and out of a staging vector.  nullptr: no.
    virtual uint8_t* mapped() { return nullptr; }
};

// In-memory disk with StackDisk's semantics (stack_disk.hpp:19-44: out-of-range accesses
// fail whole; read checks bounds, then capacity).  Storage is heap-allocated.
template <size_t power = 22> class StackDisk : public IDisk {
public:
    StackDisk()
        : _data(size_t(1) << power, 0)
    {
    }
    size_t size() override { return _data.size(); }
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
    uint8_t* image() { return _data.data(); }
    uint8_t* mapped() override { return _data.data(); }

private:
    std::vector<uint8_t> _data;
};

// File-backed disk with FileDisk's interface and checks (file_disk.hpp, file_disk.cpp:8-101:
// open an existing file / create a zero-filled one of a fixed size; read checks open, bounds,
// then capacity; write checks open and bounds), over a shared mmap of the file instead of
// fstream seek + read / write.  The mapping is page-locked for the engine when the
// HIP runtime allows it (ppfs_ecc_host_register; a file mapping it cannot pin stays pageable), so
// the batch calls DMA straight between the page cache and HBM.
class MappedFileDisk : public IDisk {
public:
    MappedFileDisk() = default;
    ~MappedFileDisk() override { close(); }
    MappedFileDisk(const MappedFileDisk&) = delete;
    MappedFileDisk& operator=(const MappedFileDisk&) = delete;

    expected<void> open(const std::string& path)
    {
        close();
        const int fd = ::open(path.c_str(), O_RDWR);
        if (fd < 0)
            return unexpected(FsError::Disk_IOError);
        struct stat st;
        if (::fstat(fd, &st) != 0) {
            ::close(fd);
            return unexpected(FsError::Disk_IOError);
        }
        _size = (size_t)st.st_size;
        if (_size) {
            void* m = ::mmap(nullptr, _size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
            if (m == MAP_FAILED) {
                ::close(fd);
                _size = 0;
                return unexpected(FsError::Disk_IOError);
            }
            _map = (uint8_t*)m;
            _pinned = ppfs_ecc_host_register(_map, _size) == 0;
        }
        _fd = fd;
        return {};
    }
    expected<void> create(const std::string& path, size_t size)
    {
        if (_fd >= 0)
            return unexpected(FsError::Disk_InvalidRequest); // file_disk.cpp:37-38
        const int fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd < 0)
            return unexpected(FsError::Disk_IOError);
        const bool ok = ::ftruncate(fd, (off_t)size) == 0;
        ::close(fd);
        if (!ok)
            return unexpected(FsError::Disk_IOError);
        return open(path);
    }
    void close()
    {
        if (_map) {
            if (_pinned)
                (void)ppfs_ecc_host_unregister(_map);
            ::msync(_map, _size, MS_SYNC);
            ::munmap(_map, _size);
        }
        if (_fd >= 0)
            ::close(_fd);
        _map = nullptr;
        _fd = -1;
        _size = 0;
        _pinned = false;
    }
    size_t size() override { return _size; }
    bool pinned() const { return _pinned; }
    uint8_t* mapped() override { return _map; }
    expected<void> read(size_t address, size_t size, static_vector<uint8_t>& data) override
    {
        if (_fd < 0)
            return unexpected(FsError::Disk_IOError);
        if (address + size > _size)
            return unexpected(FsError::Disk_OutOfBounds);
        if (data.capacity() < size)
            return unexpected(FsError::Disk_InvalidRequest);
        data.resize(size);
        if (size)
            std::memcpy(data.data(), _map + address, size);
        return {};
    }
    expected<size_t> write(size_t address, const static_vector<uint8_t>& data) override
    {
        if (_fd < 0)
            return unexpected(FsError::Disk_IOError);
        if (address + data.size() > _size)
            return unexpected(FsError::Disk_OutOfBounds);
        if (data.size())
            std::memcpy(_map + address, data.data(), data.size());
        return data.size();
    }

private:
    int _fd = -1;
    uint8_t* _map = nullptr;
    size_t _size = 0;
    bool _pinned = false;
};

// ------------------------------------------------------------------------------------------
// Logger: block devices emit only ErrorCorrectionEvent (rs:171-173, hamming:53-57)
// ------------------------------------------------------------------------------------------
struct ErrorCorrectionEvent {
    std::string codec;
    block_index_t block_index;
    ErrorCorrectionEvent(std::string c, block_index_t b)
        : codec(std::move(c))
        , block_index(b)
    {
    }
};

class Logger {
public:
    virtual ~Logger() = default;
    virtual void logEvent(const ErrorCorrectionEvent& e) { events.push_back(e); }
    std::vector<ErrorCorrectionEvent> events;
};

// ------------------------------------------------------------------------------------------
// CrcPolynomial (crc_polynomial.cpp:7-54)
// ------------------------------------------------------------------------------------------
class CrcPolynomial {
public:
    static CrcPolynomial MsgExplicit(uint64_t p) { return CrcPolynomial(p); }
    static CrcPolynomial MsgImplicit(uint64_t p) { return CrcPolynomial(ppfs_ecc_crc_implicit_to_explicit(p)); }
    uint64_t getExplicitPolynomial() const { return _p; }
    uint64_t getImplicitPolynomial() const { return _p >> 1; }
    int getDegree() const
    {
        int n = -1;
        for (uint64_t v = _p; v; v >>= 1)
            ++n;
        return n;
    }

private:
    explicit CrcPolynomial(uint64_t p)
        : _p(p)
    {
    }
    uint64_t _p;
};

// ------------------------------------------------------------------------------------------
// Engine handle (one codec context on one GPU)
// ------------------------------------------------------------------------------------------
class EccEngine {
public:
    EccEngine(uint32_t type, uint32_t block_size, uint32_t t, uint64_t poly, int device)
    {
        ppfs_ecc_params p {};
        p.ecc_type = type;
        p.block_size = block_size;
        p.rs_correctable_bytes = t;
        p.crc_polynomial = poly;
        // the reference's constructors cannot fail: a device whose engine could not be created
        // (no GPU, bad parameters) reports Disk_IOError from every call instead -- no CPU fallback
        const int rc = ppfs_ecc_create(&p, device, &_ctx);
        if (rc != 0 || !_ctx) {
            std::fprintf(stderr, "ppfs_gpu: ppfs_ecc_create failed (%d): %s\n", rc, ppfs_ecc_last_error());
            _ctx = nullptr;
        }
    }
    ~EccEngine() { ppfs_ecc_destroy(_ctx); }
    EccEngine(const EccEngine&) = delete;
    EccEngine& operator=(const EccEngine&) = delete;
    size_t raw() const { return ppfs_ecc_raw_block_size(_ctx); }
    size_t data() const { return ppfs_ecc_data_size(_ctx); }
    ppfs_ecc_ctx* ctx() const { return _ctx; }
    bool valid() const { return _ctx != nullptr; }
    // An engine call's return code: 0 -> true; else the ABI's message goes to stderr and the
    // caller returns FsError::Disk_IOError (the reference's code for a failed device operation)
    static bool ok(int rc, const char* what)
    {
        if (rc != 0) {
            std::fprintf(stderr, "ppfs_gpu: %s failed (%d): %s\n", what, rc, ppfs_ecc_last_error());
            return false;
        }
        return true;
    }

private:
    ppfs_ecc_ctx* _ctx = nullptr;
};

// ------------------------------------------------------------------------------------------
// IBlockDevice
// ------------------------------------------------------------------------------------------
class IBlockDevice {
public:
    virtual ~IBlockDevice() = default;
    virtual expected<size_t> writeBlock(const static_vector<std::uint8_t>& data, DataLocation data_location) = 0;
    virtual expected<void> readBlock(DataLocation data_location, size_t bytes_to_read, static_vector<uint8_t>& data)
        = 0;
    virtual size_t rawBlockSize() const = 0;
    virtual size_t dataSize() const = 0;
    virtual size_t numOfBlocks() const = 0;
    virtual expected<void> formatBlock(unsigned int block_index) = 0;

    // Batch extension: whole blocks [first, first + count).  out: count * dataSize() bytes;
    // err (may be null): per block 0 or the FsError the per-block call returns.  The call
    // itself fails only when the range cannot be read from / written to the disk.
    virtual expected<void> readBlocks(block_index_t first, size_t count, uint8_t* out, uint8_t* err) = 0;
    virtual expected<void> writeBlocks(block_index_t first, size_t count, const uint8_t* payloads, uint8_t* err)
        = 0;

    // List extension: whole blocks idx[0 .. count), in any order -- what FileIO's BlockIndexIterator
    // loop (file_io.cpp:27-35, 53-69) collects for a fragmented file.  Equal to the per-block calls
    // made in list order (a block listed twice is seen the second time as the first left it); out,
    // payloads and err are in list order, err (may be null) as readBlocks.  The default is that
    // per-block loop; the codecs run one engine call per list.
    virtual expected<void> readBlockList(const block_index_t* idx, size_t count, uint8_t* out, uint8_t* err)
    {
        const size_t ds = dataSize();
        for (size_t i = 0; i < count; ++i) {
            static_vector<uint8_t> v(out + i * ds, ds, 0);
            auto r = readBlock(DataLocation((int)idx[i], 0), ds, v);
            if (!r)
                std::memset(out + i * ds, 0, ds);
            if (err)
                err[i] = r ? 0 : (uint8_t)r.error();
        }
        return {};
    }
    virtual expected<void> writeBlockList(const block_index_t* idx, size_t count, const uint8_t* payloads, uint8_t* err)
    {
        const size_t ds = dataSize();
        for (size_t i = 0; i < count; ++i) {
            static_vector<uint8_t> v(const_cast<uint8_t*>(payloads + i * ds), ds, ds);
            auto r = writeBlock(v, DataLocation((int)idx[i], 0));
            if (err)
                err[i] = r ? 0 : (uint8_t)r.error();
        }
        return {};
    }

    // Extent extension: n byte ranges (block, offset, length) -- the form of FileIO::readFile /
    // writeFile (file_io.cpp:24-42, 50-88: the first block from offset % dataSize(), the last one up to
    // where the bytes run out) and of the few bytes the inode table, bitmap and directory code write at
    // DataLocation{block, offset}.  Entry i is readBlock({block, offset}, length) into
    // out[pos, pos + len) / writeBlock(in[pos, pos + len), {block, offset}), len = min(length,
    // dataSize() - offset), the entries taken in list order.  err (may be null): per entry 0 or the
    // FsError of the per-block call; a failed read's bytes become zeros.  An entry whose offset is past
    // dataSize(), whose bytes do not fit the packed buffer or whose block index is no int gets
    // Disk_OutOfBounds and touches nothing.
    // This per-block loop is the definition; the codecs run one engine call per batch.
    // DataLocation::block_index is an int: a block index that is none (0xFFFFFFFF, a caller's -1) never
    // reaches the per-block calls, where it would turn into an address before the disk's first byte.
    static bool extent_fits(const ppfs_ecc_extent& x, size_t ds, size_t buf_bytes, size_t& len)
    {
        if (x.offset > ds || x.block > 0x7FFFFFFFu)
            return false;
        len = std::min<size_t>(x.length, ds - x.offset);
        return x.pos <= buf_bytes && len <= buf_bytes - x.pos;
    }
    virtual expected<void> readExtents(const ppfs_ecc_extent* ext, size_t n, uint8_t* out, size_t out_bytes, uint8_t* err)
    {
        const size_t ds = dataSize();
        for (size_t i = 0; i < n; ++i) {
            size_t len = 0;
            FsError e = FsError::Disk_OutOfBounds;
            bool failed = !extent_fits(ext[i], ds, out_bytes, len);
            if (!failed) {
                static_vector<uint8_t> v(out + ext[i].pos, len, 0);
                auto r = readBlock(DataLocation((int)ext[i].block, ext[i].offset), len, v);
                if (!r) {
                    failed = true;
                    e = r.error();
                    if (e != FsError::Disk_OutOfBounds)
                        std::memset(out + ext[i].pos, 0, len);
                }
            }
            if (err)
                err[i] = failed ? (uint8_t)e : 0;
        }
        return {};
    }
    virtual expected<void> writeExtents(const ppfs_ecc_extent* ext, size_t n, const uint8_t* in, size_t in_bytes, uint8_t* err)
    {
        const size_t ds = dataSize();
        for (size_t i = 0; i < n; ++i) {
            size_t len = 0;
            FsError e = FsError::Disk_OutOfBounds;
            bool failed = !extent_fits(ext[i], ds, in_bytes, len);
            if (!failed) {
                static_vector<uint8_t> v(const_cast<uint8_t*>(in + ext[i].pos), len, len);
                auto r = writeBlock(v, DataLocation((int)ext[i].block, ext[i].offset));
                if (!r) {
                    failed = true;
                    e = r.error();
                }
            }
            if (err)
                err[i] = failed ? (uint8_t)e : 0;
        }
        return {};
    }

    // Whole-image scrub extension: the disk and log effect of
    // readBlock({i, 0}, dataSize()) for i in [first, first + count), in order, without the
    // payloads.  counts (may be null): blocks ok / corrected / failed; err as readBlocks.
    virtual expected<void> scrub(block_index_t first, size_t count, size_t* counts, uint8_t* err)
    {
        std::vector<uint8_t> out(count * dataSize()), e(count);
        auto r = readBlocks(first, count, out.data(), e.data());
        if (!r)
            return r;
        size_t failed = 0;
        for (uint8_t x : e)
            failed += x != 0;
        if (counts) {
            counts[0] = count - failed;
            counts[1] = 0;
            counts[2] = failed;
        }
        if (err)
            std::memcpy(err, e.data(), count);
        return {};
    }

    // Scrub of named blocks only (ppfs_ecc.h ppfs_ecc_scrub_list_* / ppfs_ecc_scrub_allocated_*): the disk and
    // log effect of readBlock({b, 0}, dataSize()) for the blocks named, without the payloads.  counts (may be
    // null) is overwritten.  These per-block loops are the definition; the codecs run one engine call.
    //   scrubList       the blocks idx[0 .. n) in list order; err (may be null) as readBlockList.  This default
    //                   cannot tell a corrected block from a clean one (both count as ok); the codecs can.
    //   scrubAllocated  the blocks first_data_block + j whose bit j is set in the on-disk bitmap (lib/bitmap/src/
    //                   bitmap.cpp) of nbits bits that starts at bitmap_block: first the bitmap's own
    //                   blocks_spanned(nbits) blocks (bitmap_err, may be null, and the bitmap_* counts), then the
    //                   allocated blocks in ascending order.  All bits of a bitmap block that cannot be read count
    //                   as set.  err (may be null): nbits bytes, 0 or the FsError for a set bit,
    //                   PPFS_ECC_NOT_ALLOCATED (255) for a clear one, whose block is not read.
    size_t bitmapBlocks(size_t nbits) const // Bitmap::blocksSpanned (bitmap.cpp:27-31) in integer arithmetic
    {
        const size_t ds = dataSize();
        return ds ? ((nbits + 7) / 8 + ds - 1) / ds : 0;
    }
    virtual expected<void> scrubList(const block_index_t* idx, size_t n, ppfs_ecc_scrub_counts* counts, uint8_t* err)
    {
        std::vector<uint8_t> out(n * dataSize()), e(n);
        auto r = readBlockList(idx, n, out.data(), e.data());
        if (!r)
            return r;
        if (counts) {
            *counts = ppfs_ecc_scrub_counts {};
            for (uint8_t x : e)
                ++(x == 0 ? counts->ok : x == (uint8_t)FsError::Disk_OutOfBounds ? counts->out_of_range : counts->failed);
        }
        if (err && n)
            std::memcpy(err, e.data(), n);
        return {};
    }
    virtual expected<void> scrubAllocated(block_index_t bitmap_block, block_index_t first_data_block, size_t nbits,
        ppfs_ecc_scrub_counts* counts, uint8_t* err, uint8_t* bitmap_err)
    {
        const size_t ds = dataSize(), B = bitmapBlocks(nbits);
        if (ds == 0 || (uint64_t)first_data_block + nbits > (1ull << 32))
            return unexpected(FsError::Disk_OutOfBounds);
        if (counts)
            *counts = ppfs_ecc_scrub_counts {};
        if (nbits == 0)
            return {};
        std::vector<uint8_t> stream(B * ds), be(B);
        ppfs_ecc_scrub_counts bc {};
        {
            std::vector<block_index_t> bidx(B);
            for (size_t b = 0; b < B; ++b)
                bidx[b] = bitmap_block + (block_index_t)b;
            if ((size_t)bitmap_block + B > numOfBlocks())
                return unexpected(FsError::Disk_OutOfBounds);
            auto r = readBlocks(bitmap_block, B, stream.data(), be.data());
            if (!r)
                return r;
            for (uint8_t x : be)
                ++(x == 0 ? bc.bitmap_ok : bc.bitmap_failed);
        }
        if (bitmap_err)
            std::memcpy(bitmap_err, be.data(), B);
        std::vector<block_index_t> list;
        for (size_t j = 0; j < nbits; ++j)
            if (be[j / (8 * ds)] != 0 || (stream[j / 8] & (0x80u >> (j % 8))))
                list.push_back(first_data_block + (block_index_t)j);
        std::vector<uint8_t> e(list.size());
        ppfs_ecc_scrub_counts lc {};
        auto r = scrubList(list.data(), list.size(), &lc, e.data());
        if (!r)
            return r;
        if (err) {
            std::memset(err, PPFS_ECC_NOT_ALLOCATED, nbits);
            for (size_t k = 0; k < list.size(); ++k)
                err[list[k] - first_data_block] = e[k];
        }
        if (counts) {
            *counts = lc;
            counts->not_allocated = nbits - list.size();
            counts->bitmap_ok = bc.bitmap_ok;
            counts->bitmap_corrected = 0;
            counts->bitmap_failed = bc.bitmap_failed;
        }
        return {};
    }

    // File extension (ppfs_ecc.h ppfs_ecc_file_blocks_* / ppfs_ecc_read_file_*): a file read from the 64 bytes of
    // its inode that describe the index-block tree (inode.hpp:18-41).  These per-block loops are the definition:
    // the read-only BlockIndexIterator (file_io.cpp:186-463) through readBlock.  An index block is read, as
    // readBlock({b, 0}, 4 * ipb), immediately before the first requested file block under it, outer levels
    // first, each one once; the first error ends the walk.  The codecs walk the whole tree in engine calls.
    //   fileBlocks  idx[i] = the image block of file block first + i.  On an error the call returns it; the
    //               blocks before the failing one are resolved, err (may be null) holds 0 for them and the
    //               error from the failing block on.
    //   readFile    FileIO::readFile (file_io.cpp:12-44): out[0, n) = the file's bytes from offset, n =
    //               min(bytes_to_read, file_size - offset), which is the value returned.  On an error the call
    //               returns it; the bytes before the failing block are delivered, *delivered (may be null)
    //               says how many.
    struct FilePath {
        unsigned segment; // 0: direct[slot[0]]; 1, 2, 3: that many index blocks above the block; 4: past the tree
        uint64_t slot[3]; // the slot taken at each index block, from the root down
    };
    static FilePath file_path(uint64_t j, uint64_t ipb)
    {
        FilePath p { 4, { 0, 0, 0 } };
        if (j < 12) {
            p.segment = 0;
            p.slot[0] = j;
            return p;
        }
        uint64_t s = j - 12;
        if (s < ipb) {
            p.segment = 1;
            p.slot[0] = s;
            return p;
        }
        s -= ipb;
        if (s < ipb * ipb) {
            p.segment = 2;
            p.slot[0] = s / ipb;
            p.slot[1] = s % ipb;
            return p;
        }
        s -= ipb * ipb;
        if (s < ipb * ipb * ipb) {
            p.segment = 3;
            p.slot[0] = s / (ipb * ipb);
            p.slot[1] = (s / ipb) % ipb;
            p.slot[2] = s % ipb;
        }
        return p;
    }
    static uint64_t file_occupied(const ppfs_ecc_file& file, size_t ds) { return ds ? ((uint64_t)file.file_size + ds - 1) / ds : 0; }
    // The iterator: the index block loaded at each depth and which one it is.  File blocks are asked for in
    // ascending order, so one block per depth is all the walk ever holds.
    class FileWalk {
    public:
        FileWalk(IBlockDevice& dev, const ppfs_ecc_file& file)
            : _dev(dev)
            , _file(file)
            , _ds(dev.dataSize())
            , _ipb(_ds / 4)
        {
        }
        expected<block_index_t> block(uint64_t j)
        {
            const FilePath p = file_path(j, _ipb);
            if (j >= file_occupied(_file, _ds) || p.segment > 3)
                return unexpected(FsError::FileIO_OutOfBounds);
            if (p.segment == 0)
                return _file.direct[j];
            block_index_t pointer = p.segment == 1 ? _file.indirect : p.segment == 2 ? _file.doubly_indirect : _file.trebly_indirect;
            uint64_t id = p.segment; // which index block: the segment and the slots taken so far
            for (unsigned d = 0; d < p.segment; ++d) {
                if (!_have[d] || _id[d] != id) {
                    _entries[d].assign(_ds, 0);
                    static_vector<uint8_t> v(_entries[d].data(), _ds, 0);
                    _have[d] = false;
                    auto r = _dev.readBlock(DataLocation((int)pointer, 0), 4 * _ipb, v);
                    if (!r)
                        return unexpected(r.error());
                    _have[d] = true;
                    _id[d] = id;
                }
                const uint8_t* e = _entries[d].data() + 4 * p.slot[d];
                pointer = (block_index_t)e[0] | (block_index_t)e[1] << 8 | (block_index_t)e[2] << 16 | (block_index_t)e[3] << 24;
                id = id * (_ipb + 1) + p.slot[d] + 1;
            }
            return pointer;
        }

    private:
        IBlockDevice& _dev;
        const ppfs_ecc_file& _file;
        size_t _ds, _ipb;
        bool _have[3] = { false, false, false };
        uint64_t _id[3] = { 0, 0, 0 };
        std::vector<uint8_t> _entries[3];
    };
    virtual expected<void> fileBlocks(const ppfs_ecc_file& file, uint64_t first, size_t count, block_index_t* idx, uint8_t* err)
    {
        FileWalk walk(*this, file);
        for (size_t i = 0; i < count; ++i) {
            auto r = walk.block(first + i);
            if (!r) {
                if (err)
                    std::memset(err + i, (int)(uint8_t)r.error(), count - i);
                return unexpected(r.error());
            }
            idx[i] = *r;
            if (err)
                err[i] = 0;
        }
        return {};
    }
    virtual expected<size_t> readFile(const ppfs_ecc_file& file, size_t offset, size_t bytes_to_read, uint8_t* out,
        size_t* delivered = nullptr)
    {
        const size_t ds = dataSize();
        if (delivered)
            *delivered = 0;
        if (bytes_to_read == 0)
            return (size_t)0;
        if (ds == 0 || offset >= file.file_size)
            return unexpected(FsError::FileIO_OutOfBounds);
        const size_t n = std::min<size_t>(bytes_to_read, file.file_size - offset);
        FileWalk walk(*this, file);
        size_t done = 0;
        for (uint64_t j = offset / ds; done < n; ++j) {
            auto b = walk.block(j);
            if (!b)
                return unexpected(b.error());
            const size_t off = done == 0 ? offset % ds : 0, len = std::min(ds - off, n - done);
            static_vector<uint8_t> v(out + done, len, 0);
            auto r = readBlock(DataLocation((int)*b, (int)off), len, v);
            if (!r)
                return unexpected(r.error());
            done += len;
            if (delivered)
                *delivered = done;
        }
        return n;
    }

    // Batch extension (ppfs_ecc.h ppfs_ecc_files_blocks_* / ppfs_ecc_read_files_*): many (inode, offset, length)
    // in one call -- a directory scan, a backup.  By definition the loop over readFile, in batch order; the
    // codecs walk all the files' trees in one engine call.  Per read: ok and `bytes` (the value readFile
    // returns) or `error`, and `delivered` as readFile reports it.
    struct FileRead {
        ppfs_ecc_file file;
        size_t offset, bytes_to_read;
        uint8_t* out; // room for min(bytes_to_read, file_size - offset) bytes
        bool ok;
        FsError error;
        size_t bytes, delivered;
    };
    virtual void readFiles(FileRead* reads, size_t n)
    {
        for (size_t i = 0; i < n; ++i)
            read_one(reads[i], readFile(reads[i].file, reads[i].offset, reads[i].bytes_to_read, reads[i].out, &reads[i].delivered));
    }

    // Inode extension (ppfs_ecc.h ppfs_ecc_read_inodes_*): n inode numbers of one inode table in one call -- the
    // children of a directory.  By definition the per-inode loop, InodeManager::get (inode_manager.cpp:127-138):
    // Bitmap::getBit (bitmap.cpp:8-25, 87-101), a one-byte readBlock of the inode bitmap, in which a SET bit means
    // free (InodeManager_NotFound); then _readInode (:56-89), the 81 packed bytes cut at block boundaries by a
    // clamping readBlock.  The first error ends that inode.  table.check_bitmap == 0 skips the bit's read, not the
    // range check.  The codecs read the whole batch in one engine call.
    using InodeTable = ppfs_ecc_inode_table;
#pragma pack(push, 1)
    struct PackedInode { // inode.hpp:18-41
        uint64_t time_creation, time_modified;
        ppfs_ecc_file file; // direct[12], indirect, doubly_indirect, trebly_indirect, file_size
        uint8_t type;       // 0 file, 1 directory
    };
#pragma pack(pop)
    static_assert(sizeof(PackedInode) == 81, "the packed Inode");
    struct InodeRead {
        bool ok;
        FsError error;
        PackedInode inode; // zero unless ok
    };
    expected<bool> inodeBit(const InodeTable& table, uint32_t bit_index)
    {
        if (bit_index >= table.total_inodes)
            return unexpected(FsError::Bitmap_IndexOutOfRange);
        const size_t ds = dataSize(), byte = bit_index / 8;
        uint8_t b = 0;
        static_vector<uint8_t> v(&b, 1, 0);
        auto r = readBlock(DataLocation((int)(table.bitmap_block + byte / ds), byte % ds), 1, v);
        if (!r)
            return unexpected(r.error());
        return ((b >> (7 - bit_index % 8)) & 1) > 0;
    }
    expected<void> readInode(const InodeTable& table, uint32_t index, PackedInode& inode)
    {
        const size_t ds = dataSize(), size = sizeof(PackedInode);
        uint8_t* bytes = reinterpret_cast<uint8_t*>(&inode);
        size_t bytes_read = 0;
        DataLocation start((int)(table.table_block + (uint64_t)index * size / ds), (size_t)((uint64_t)index * size % ds));
        if (ds - start.offset < size) { // does not fit in one block: the unaligned part first
            static_vector<uint8_t> v(bytes, size, 0);
            auto r = readBlock(start, size, v);
            if (!r)
                return unexpected(r.error());
            start.offset = 0;
            start.block_index++;
            bytes_read += v.size();
        }
        while (bytes_read < size) {
            const size_t bytes_left = size - bytes_read;
            static_vector<uint8_t> v(bytes + bytes_read, bytes_left, 0);
            auto r = readBlock(start, bytes_left, v);
            if (!r)
                return unexpected(r.error());
            bytes_read += v.size();
            start.block_index++;
        }
        return {};
    }
    virtual void readInodes(const InodeTable& table, const uint32_t* numbers, size_t n, InodeRead* out)
    {
        for (size_t j = 0; j < n; ++j) {
            InodeRead& r = out[j];
            r = InodeRead {};
            auto fail = [&](FsError e) { r.error = e; };
            if (dataSize() == 0) {
                fail(FsError::Disk_InvalidRequest);
                continue;
            }
            if (table.check_bitmap) {
                auto is_free = inodeBit(table, numbers[j]);
                if (!is_free) {
                    fail(is_free.error());
                    continue;
                }
                if (*is_free) {
                    fail(FsError::InodeManager_NotFound);
                    continue;
                }
            } else if (numbers[j] >= table.total_inodes) {
                fail(FsError::Bitmap_IndexOutOfRange);
                continue;
            }
            PackedInode inode {};
            auto got = readInode(table, numbers[j], inode);
            if (!got) {
                fail(got.error());
                continue;
            }
            r.ok = true;
            r.inode = inode;
        }
    }

    // Lookup extension (ppfs_ecc.h ppfs_ecc_lookup_*): nq (directory, key) queries over ndirs directories in one call
    // -- one path component of many paths, the uniqueness test before many creates.  By definition the loop of
    // DirectoryManager::getInodeByName (directory_manager.cpp:135-163) for lookupNames and of removeEntry's search
    // (:67-90, up to and including the found_entry decision) for lookupInodes: _readDirectoryData (:165-187), a
    // readFile of at most 256 DirectoryEntry records, then _findEntryByName (:189-199) / _findEntryByInode (:201-210).
    // A name is a 128-byte record, NUL-terminated within its first 124 bytes (else it matches nothing).  DEVIATION:
    // an entry whose 124 name bytes hold no NUL matches nothing; the reference's strlen would run on into the next
    // entry.  The codecs read every directory once and whole in one engine call.
    static constexpr size_t kDirEntryBytes = 128, kDirEntryBatch = 256, kDirNameBytes = 124;
    struct Lookup {
        uint32_t dir;        // a number into the call's directories
        uint32_t key;        // lookupInodes: the inode number
        const uint8_t* name; // lookupNames: the 128-byte record
        bool ok;
        FsError error; // the failing block's, PpFS_NotFound (names) or DirectoryManager_NotFound (inodes)
        uint32_t inode, entry; // 0xFFFFFFFF unless ok
    };
    // the position of the first NUL among the first cap bytes, cap when there is none
    static size_t lookup_strnlen(const uint8_t* p, size_t cap)
    {
        const void* at = std::memchr(p, 0, cap);
        return at ? (size_t)((const uint8_t*)at - p) : cap;
    }
    void lookup_loop(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq, bool by_name)
    {
        std::vector<uint8_t> buffer(kDirEntryBatch * kDirEntryBytes);
        for (size_t q = 0; q < nq; ++q) {
            Lookup& r = queries[q];
            r.ok = false;
            r.inode = r.entry = 0xFFFFFFFFu;
            r.error = by_name ? FsError::PpFS_NotFound : FsError::DirectoryManager_NotFound;
            if (r.dir >= ndirs) {
                r.error = FsError::DirectoryManager_InvalidRequest;
                continue;
            }
            const ppfs_ecc_file& dir = dirs[r.dir];
            const size_t L = by_name ? lookup_strnlen(r.name, 128) : 0;
            const size_t num_entries = dir.file_size / kDirEntryBytes;
            size_t checked = 0;
            bool done = false;
            while (checked < num_entries && !done) {
                const size_t size = std::min(kDirEntryBatch, num_entries - checked);
                auto read_res = readFile(dir, checked * kDirEntryBytes, size * kDirEntryBytes, buffer.data());
                if (!read_res) {
                    r.error = read_res.error();
                    break;
                }
                const size_t got = *read_res / kDirEntryBytes;
                for (size_t i = 0; i < got && !done; ++i) {
                    const uint8_t* e = buffer.data() + i * kDirEntryBytes;
                    uint32_t inode;
                    std::memcpy(&inode, e, 4);
                    const bool hit = by_name ? L < kDirNameBytes && lookup_strnlen(e + 4, kDirNameBytes) == L && std::memcmp(e + 4, r.name, L) == 0
                                             : inode == r.key;
                    if (hit) {
                        r.ok = done = true;
                        r.error = FsError {};
                        r.inode = inode;
                        r.entry = (uint32_t)(checked + i);
                    }
                }
                checked += got;
                if (got == 0)
                    break;
            }
        }
    }
    virtual void lookupNames(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq) { lookup_loop(dirs, ndirs, queries, nq, true); }
    virtual void lookupInodes(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq) { lookup_loop(dirs, ndirs, queries, nq, false); }

    // The mirror (ppfs_ecc.h ppfs_ecc_write_inodes_*): n inodes written into one inode table in one call -- what
    // follows a batch of file writes.  By definition the per-inode loop, InodeManager::update (inode_manager.cpp:
    // 142-159): Bitmap::getBit as above, then _writeInode (:20-54), the 81 packed bytes cut at block boundaries by a
    // clamping writeBlock.  The first error ends that inode.  The codecs write the whole batch in one engine call.
    struct InodeWrite {
        bool ok;
        FsError error; // meaningful unless ok (Bitmap_IndexOutOfRange is FsError 0)
    };
    expected<void> writeInode(const InodeTable& table, uint32_t index, const PackedInode& inode)
    {
        const size_t ds = dataSize(), size = sizeof(PackedInode);
        uint8_t* data = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(&inode)); // static_vector only reads it
        size_t bytes_written = 0;
        DataLocation start((int)(table.table_block + (uint64_t)index * size / ds), (size_t)((uint64_t)index * size % ds));
        if (ds - start.offset < size) { // does not fit in one block: the unaligned part first
            static_vector<uint8_t> v(data, size, size);
            auto r = writeBlock(v, start);
            if (!r)
                return unexpected(r.error());
            bytes_written += *r;
            start.offset = 0;
            start.block_index++;
        }
        while (bytes_written < size) {
            const size_t bytes_left = size - bytes_written;
            static_vector<uint8_t> v(data + bytes_written, bytes_left, bytes_left);
            auto r = writeBlock(v, start);
            if (!r)
                return unexpected(r.error());
            start.block_index++;
            bytes_written += *r;
        }
        return {};
    }
    virtual void writeInodes(const InodeTable& table, const uint32_t* numbers, size_t n, const PackedInode* inodes, InodeWrite* out)
    {
        for (size_t j = 0; j < n; ++j) {
            InodeWrite& r = out[j];
            r = InodeWrite {};
            if (dataSize() == 0) {
                r.error = FsError::Disk_InvalidRequest;
                continue;
            }
            if (table.check_bitmap) {
                auto is_free = inodeBit(table, numbers[j]);
                if (!is_free) {
                    r.error = is_free.error();
                    continue;
                }
                if (*is_free) {
                    r.error = FsError::InodeManager_NotFound;
                    continue;
                }
            } else if (numbers[j] >= table.total_inodes) {
                r.error = FsError::Bitmap_IndexOutOfRange;
                continue;
            }
            auto put = writeInode(table, numbers[j], inodes[j]);
            if (put)
                r.ok = true;
            else
                r.error = put.error();
        }
    }

    // Write extension (ppfs_ecc.h ppfs_ecc_write_file_* / ppfs_ecc_write_files_*): the in-place case of
    // FileIO::writeFile (file_io.cpp:46-104).  The range must lie inside the file as the inode describes it --
    // offset + n <= file_size, else FileIO_OutOfBounds as readFile reports a range past the end; nothing is
    // allocated, nothing grows, no inode is updated.  The per-block loop is the definition: the walk above, one
    // writeBlock per data block, the first error ends it.  The value returned is n; on an error the call returns
    // it and *written (may be null) says how many bytes were written before the failing block.  n == 0 touches
    // nothing.  The codecs write the whole range, or a batch of them, in engine calls.
    virtual expected<size_t> writeFile(const ppfs_ecc_file& file, size_t offset, const uint8_t* in, size_t n, size_t* written = nullptr)
    {
        const size_t ds = dataSize();
        if (written)
            *written = 0;
        if (n == 0)
            return (size_t)0;
        if (ds == 0 || offset + n < offset || offset + n > file.file_size)
            return unexpected(FsError::FileIO_OutOfBounds);
        FileWalk walk(*this, file);
        size_t done = 0;
        for (uint64_t j = offset / ds; done < n; ++j) {
            auto b = walk.block(j);
            if (!b)
                return unexpected(b.error());
            const size_t off = done == 0 ? offset % ds : 0, len = std::min(ds - off, n - done);
            static_vector<uint8_t> v(const_cast<uint8_t*>(in) + done, len, len);
            auto r = writeBlock(v, DataLocation((int)*b, (int)off));
            if (!r)
                return unexpected(r.error());
            done += len;
            if (written)
                *written = done;
        }
        return n;
    }
    // By definition the loop over writeFile, in batch order.  Per write: ok and `bytes` (the value writeFile
    // returns) or `error`, and `written` as writeFile reports it.
    struct FileWrite {
        ppfs_ecc_file file;
        size_t offset;
        const uint8_t* in;
        size_t n;
        bool ok;
        FsError error;
        size_t bytes, written;
    };
    virtual void writeFiles(FileWrite* writes, size_t n)
    {
        for (size_t i = 0; i < n; ++i)
            write_one(writes[i], writeFile(writes[i].file, writes[i].offset, writes[i].in, writes[i].n, &writes[i].written));
    }

protected:
    static void read_one(FileRead& r, const expected<size_t>& got)
    {
        r.ok = (bool)got;
        r.error = got ? FsError {} : got.error();
        r.bytes = got ? *got : 0;
    }
    static void write_one(FileWrite& w, const expected<size_t>& got)
    {
        w.ok = (bool)got;
        w.error = got ? FsError {} : got.error();
        w.bytes = got ? *got : 0;
    }
};

// The entries of a FileIO::readFile / writeFile walk (file_io.cpp:24-42, 50-88) over the blocks
// idx[0 .. count), from the block that holds the first byte on: the first block from
// offset_in_first_block = offset % dataSize(), whole blocks after it, the last one up to where the
// nbytes run out; pos is the running sum, so the packed buffer is the file range itself.  One
// readExtents / writeExtents call then does what the loop's per-block calls do.
inline std::vector<ppfs_ecc_extent> file_extents(const block_index_t* idx, size_t count, size_t offset_in_first_block,
    size_t nbytes, size_t data_size)
{
    std::vector<ppfs_ecc_extent> out;
    if (data_size == 0 || offset_in_first_block >= data_size)
        return out;
    size_t done = 0;
    for (size_t k = 0; k < count && done < nbytes; ++k) {
        const size_t off = k == 0 ? offset_in_first_block : 0;
        const size_t len = std::min(data_size - off, nbytes - done);
        out.push_back(ppfs_ecc_extent { (uint64_t)done, idx[k], (uint16_t)off, (uint16_t)len });
        done += len;
    }
    return out;
}

namespace detail {
    inline expected<void> disk_read(IDisk& d, size_t addr, size_t n, uint8_t* dst)
    {
        static_vector<uint8_t> v(dst, n);
        return d.read(addr, n, v);
    }
    inline expected<size_t> disk_write(IDisk& d, size_t addr, const uint8_t* src, size_t n)
    {
        static_vector<uint8_t> v(const_cast<uint8_t*>(src), n, n);
        return d.write(addr, v);
    }
} // namespace detail

class RawBlockDevice : public IBlockDevice {
public:
    RawBlockDevice(size_t block_size, IDisk& disk)
        : _bs(block_size)
        , _disk(disk)
    {
    }
    size_t rawBlockSize() const override { return _bs; }
    size_t dataSize() const override { return _bs; }
    size_t numOfBlocks() const override { return _disk.size() / _bs; }
    expected<void> formatBlock(unsigned int) override { return {}; }
    expected<size_t> writeBlock(const static_vector<std::uint8_t>& data, DataLocation loc) override
    {
        const size_t to_write = std::min(data.size(), _bs - loc.offset);
        auto r = detail::disk_write(_disk, loc.block_index * _bs + loc.offset, data.data(), to_write);
        if (!r)
            return unexpected(r.error());
        return to_write;
    }
    expected<void> readBlock(DataLocation loc, size_t n, static_vector<uint8_t>& data) override
    {
        const size_t to_read = std::min(n, _bs - loc.offset);
        return _disk.read(loc.block_index * _bs + loc.offset, to_read, data);
    }
    expected<void> readBlocks(block_index_t first, size_t count, uint8_t* out, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        return detail::disk_read(_disk, (size_t)first * _bs, count * _bs, out);
    }
    expected<void> writeBlocks(block_index_t first, size_t count, const uint8_t* payloads, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        auto r = detail::disk_write(_disk, (size_t)first * _bs, payloads, count * _bs);
        if (!r)
            return unexpected(r.error());
        return {};
    }
    // lists: one plain copy per entry
    expected<void> readBlockList(const block_index_t* idx, size_t count, uint8_t* out, uint8_t* err) override
    {
        for (size_t i = 0; i < count; ++i) {
            auto r = detail::disk_read(_disk, (size_t)idx[i] * _bs, _bs, out + i * _bs);
            if (!r)
                std::memset(out + i * _bs, 0, _bs);
            if (err)
                err[i] = r ? 0 : (uint8_t)r.error();
        }
        return {};
    }
    expected<void> writeBlockList(const block_index_t* idx, size_t count, const uint8_t* payloads, uint8_t* err) override
    {
        for (size_t i = 0; i < count; ++i) {
            auto r = detail::disk_write(_disk, (size_t)idx[i] * _bs, payloads + i * _bs, _bs);
            if (err)
                err[i] = r ? 0 : (uint8_t)r.error();
        }
        return {};
    }

    // extents: one plain copy per entry
    expected<void> readExtents(const ppfs_ecc_extent* ext, size_t n, uint8_t* out, size_t out_bytes, uint8_t* err) override
    {
        for (size_t i = 0; i < n; ++i) {
            size_t len = 0;
            FsError e = FsError::Disk_OutOfBounds;
            bool failed = !extent_fits(ext[i], _bs, out_bytes, len);
            if (!failed) {
                auto r = detail::disk_read(_disk, (size_t)ext[i].block * _bs + ext[i].offset, len, out + ext[i].pos);
                if (!r) {
                    failed = true;
                    e = r.error();
                }
            }
            if (err)
                err[i] = failed ? (uint8_t)e : 0;
        }
        return {};
    }
    expected<void> writeExtents(const ppfs_ecc_extent* ext, size_t n, const uint8_t* in, size_t in_bytes, uint8_t* err) override
    {
        for (size_t i = 0; i < n; ++i) {
            size_t len = 0;
            FsError e = FsError::Disk_OutOfBounds;
            bool failed = !extent_fits(ext[i], _bs, in_bytes, len);
            if (!failed) {
                auto r = detail::disk_write(_disk, (size_t)ext[i].block * _bs + ext[i].offset, in + ext[i].pos, len);
                if (!r) {
                    failed = true;
                    e = r.error();
                }
            }
            if (err)
                err[i] = failed ? (uint8_t)e : 0;
        }
        return {};
    }

private:
    size_t _bs;
    IDisk& _disk;
};

// Shared plumbing of the four ECC codecs: the per-block RMW path and the batched path both go
// through the engine's host entry points (pinned staging, chunked, H2D/kernel/D2H overlapped).
class EngineBlockDevice : public IBlockDevice {
protected:
    // The steps every batch call below is made of, each in one place.

    // The mapped disk image when a batch call may run the engine on it in place, else null: the disk is mapped,
    // the code is no shortened RS code (whose write-back may run into the next block) and the engine exists.
    // ppfs_ecc_create gives every codec a raw block of at least one byte, so _raw == 0 says that it failed.
    // A condition only one call has (_ds, n, a file's range) stands at that call.
    uint8_t* engine_image() { return !has_spill() && _raw ? _disk.mapped() : nullptr; }

    // An engine status as the FsError byte the per-block call reports: ok and corrected are no error, and every
    // other status is the FsError's own value (the static_asserts at FsError; 255, not allocated, stays 255).
    static uint8_t status_error(uint8_t status) { return status <= PPFS_ECC_CORRECTED ? 0 : status; }

    // The status of one inode of an inode call as the per-inode loop reports it: true, or false and the FsError --
    // out of range whatever else the status says, not found for a free inode, else the status' own value.
    static bool inode_ok(const ppfs_ecc_inode_table& table, uint32_t number, uint8_t status, FsError& error)
    {
        if (status <= PPFS_ECC_CORRECTED)
            return true;
        error = number >= table.total_inodes     ? FsError::Bitmap_IndexOutOfRange
            : status == PPFS_ECC_NOT_ALLOCATED ? FsError::InodeManager_NotFound
                                               : (FsError)status_error(status);
        return false;
    }

    // The correction log of an inode call from its piece_status (1 + K slots per inode), as the loop writes it: inodes
    // in batch order, the bitmap block then the pieces up to the first failing one, each block that some access of
    // the call corrected logged where the loop first touches it.
    void inode_log(const ppfs_ecc_inode_table& table, const uint32_t* numbers, size_t n, const uint8_t* pieces)
    {
        const size_t K = 2 + 79 / _ds, W = 1 + K;
        // the accesses the loop makes for inode j, in its order: fn(block, status) until it returns false
        auto touches_of = [&](size_t j, auto fn) {
            const uint8_t* ps = pieces + j * W;
            const uint64_t i = numbers[j];
            if (ps[0] != 255 && !fn((uint64_t)table.bitmap_block + (i / 8) / _ds, ps[0]))
                return;
            for (size_t k = 0; k < K && ps[1 + k] != 255; ++k)
                if (!fn((uint64_t)table.table_block + 81 * i / _ds + k, ps[1 + k]))
                    return;
        };
        std::unordered_set<uint64_t> corrected, logged;
        for (size_t j = 0; j < n; ++j)
            touches_of(j, [&](uint64_t b, uint8_t st) {
                if (st == PPFS_ECC_CORRECTED)
                    corrected.insert(b);
                return true;
            });
        for (size_t j = 0; j < n; ++j)
            touches_of(j, [&](uint64_t b, uint8_t st) {
                if (st == PPFS_ECC_CORRECTION_ERROR || st == PPFS_ECC_OUT_OF_BOUNDS)
                    return false;
                if (corrected.count(b) && logged.insert(b).second)
                    log((block_index_t)b);
                return true;
            });
    }

    // The n statuses of an engine call as the per-block calls report them, in entry order: a correction event
    // for every status 1 at block_of(i), err[i] (err may be null) 0 or the error, and, with `payloads`, zeros
    // for a failed entry's dataSize() bytes.
    template <class BlockOf> void report(const uint8_t* status, size_t n, BlockOf block_of, uint8_t* err, uint8_t* payloads = nullptr)
    {
        for (size_t i = 0; i < n; ++i) {
            if (err)
                err[i] = status_error(status[i]);
            if (status[i] == PPFS_ECC_OK) // nearly every entry, and a scrub of a whole image walks 2^20 of them
                continue;
            if (status[i] == PPFS_ECC_CORRECTED)
                log(block_of(i));
            else if (payloads)
                std::memset(payloads + i * _ds, 0, _ds);
        }
    }
    // report's rules: entry i is block first + i / idx[i] / ext[i].block
    static auto from(block_index_t first) { return [first](size_t i) { return first + (block_index_t)i; }; }
    static auto of(const block_index_t* idx) { return [idx](size_t i) { return idx[i]; }; }
    static auto of(const ppfs_ecc_extent* ext) { return [ext](size_t i) { return ext[i].block; }; }

public:
    size_t rawBlockSize() const override { return _raw; }
    size_t dataSize() const override { return _ds; }
    size_t numOfBlocks() const override { return _raw ? _disk.size() / _raw : 0; }

    expected<void> formatBlock(unsigned int block_index) override
    {
        // rs:15-23, hamming:164-172, parity:22-29 write an all-zero raw block; crc:124-134 an
        // all-zero payload with its CRC -- the engine's encode of a zero payload is exactly that
        std::vector<uint8_t> raw(_raw, 0), zero(_ds, 0);
        if (_type == PPFS_ECC_CRC && !EccEngine::ok(ppfs_ecc_encode_host(_eng.ctx(), zero.data(), raw.data(), 1), "encode"))
            return unexpected(FsError::Disk_IOError);
        auto r = detail::disk_write(_disk, (size_t)block_index * _raw, raw.data(), _raw);
        if (!r)
            return unexpected(r.error());
        return {};
    }

    expected<void> readBlock(DataLocation loc, size_t bytes_to_read, static_vector<uint8_t>& data) override
    {
        data.resize(0);
        if (data.capacity() < bytes_to_read)
            return unexpected(FsError::Disk_InvalidRequest);
        bytes_to_read = std::min(_ds - loc.offset, bytes_to_read);
        std::vector<uint8_t> raw(_raw), dec(_ds);
        auto rr = detail::disk_read(_disk, (size_t)loc.block_index * _raw, _raw, raw.data());
        if (!rr)
            return unexpected(rr.error());
        auto fx = check_fix(loc.block_index, raw.data(), dec.data());
        if (!fx)
            return unexpected(fx.error());
        data.resize(bytes_to_read);
        std::memcpy(data.data(), dec.data() + loc.offset, bytes_to_read);
        return {};
    }

    expected<size_t> writeBlock(const static_vector<std::uint8_t>& data, DataLocation loc) override
    {
        const size_t to_write = std::min(data.size(), _ds - loc.offset);
        std::vector<uint8_t> raw(_raw), dec(_ds);
        auto rr = detail::disk_read(_disk, (size_t)loc.block_index * _raw, _raw, raw.data());
        if (!rr)
            return unexpected(rr.error());
        auto fx = check_fix(loc.block_index, raw.data(), dec.data()); // raw: the fixed old block
        if (!fx)
            return unexpected(fx.error());
        std::memcpy(dec.data() + loc.offset, data.data(), to_write);
        // encode over the old block: CRC tail bits / Hamming unused bits keep their contents
        if (!EccEngine::ok(ppfs_ecc_encode_host(_eng.ctx(), dec.data(), raw.data(), 1), "encode"))
            return unexpected(FsError::Disk_IOError);
        auto w = detail::disk_write(_disk, (size_t)loc.block_index * _raw, raw.data(), _raw);
        if (!w)
            return unexpected(w.error());
        return to_write;
    }

    // readBlock({first + i, 0}) for i in [from, count): each block's own error (e.g.
    // Disk_OutOfBounds past the disk end) in err[i], decoded payloads (zeros on error) in out --
    // the per-block contract, for ranges the batch path cannot read in one piece
    expected<void> per_block_reads(block_index_t first, size_t from, size_t count, uint8_t* out, uint8_t* err)
    {
        for (size_t i = from; i < count; ++i) {
            static_vector<uint8_t> v(out + i * _ds, _ds, 0);
            auto r = readBlock(DataLocation((int)(first + (block_index_t)i), 0), _ds, v);
            if (!r) {
                std::memset(out + i * _ds, 0, _ds);
                if (err)
                    err[i] = (uint8_t)r.error();
            }
        }
        return {};
    }

    expected<void> readBlocks(block_index_t first, size_t count, uint8_t* out, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        // Not engine_image(): that also asks for an engine, and here a device without one (_raw == 0) can be told
        // from the outside.  On the image its null-context engine call fails for an empty range too, where the
        // staged path below returns success, and the staged path makes a zero-byte disk read first.
        if (uint8_t* img = _disk.mapped(); img && !has_spill()) {
            // in place on the disk image: the engine writes corrected codewords back into it
            // (RS: whole codeword, Hamming: the flipped byte, as the reference's write-back)
            if (((size_t)first + count) * _raw > _disk.size())
                return per_block_reads(first, 0, count, out, err); // range runs off the disk
            std::vector<uint8_t> status(count);
            if (!EccEngine::ok(ppfs_ecc_decode_host(_eng.ctx(), img + (size_t)first * _raw, out, status.data(), count,
                                   1, nullptr),
                    "decode"))
                return unexpected(FsError::Disk_IOError);
            report(status.data(), count, from(first), err, out);
            return {};
        }
        size_t done = 0;
        while (done < count) {
            const size_t nb = count - done;
            const block_index_t b0 = first + (block_index_t)done;
            std::vector<uint8_t> raw(nb * _raw), fixed, status(nb), spill;
            auto rr = detail::disk_read(_disk, (size_t)b0 * _raw, nb * _raw, raw.data());
            if (!rr)
                return per_block_reads(first, done, count, out, err); // range not on the disk
            fixed = raw;
            if (has_spill())
                spill.assign(nb * spill_stride(), 0);
            if (!EccEngine::ok(ppfs_ecc_decode_host(_eng.ctx(), fixed.data(), out + done * _ds, status.data(), nb,
                                 1, spill.empty() ? nullptr : spill.data()), "decode"))
                return unexpected(FsError::Disk_IOError);
            size_t i = 0;
            for (; i < nb; ++i) {
                const block_index_t b = b0 + (block_index_t)i;
                if (const uint8_t e = status_error(status[i])) {
                    if (err)
                        err[done + i] = e;
                    std::memset(out + (done + i) * _ds, 0, _ds);
                    continue;
                }
                if (status[i] != PPFS_ECC_CORRECTED)
                    continue;
                const uint8_t* sp = spill.empty() ? nullptr : spill.data() + i * spill_stride();
                auto wb = write_back(b, raw.data() + i * _raw, fixed.data() + i * _raw, sp);
                if (!wb && err)
                    err[done + i] = (uint8_t)wb.error();
                if (sp && sp[0] && i + 1 < nb) {
                    // the reference's write-back ran past this block into the next one, which
                    // the per-block loop reads afterwards: resume from there
                    ++i;
                    break;
                }
            }
            done += i;
        }
        return {};
    }

    expected<void> writeBlocks(block_index_t first, size_t count, const uint8_t* payloads, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        if (has_spill()) {
            // shortened RS codes: an old block's write-back may spill into the next block
            // before it is read; keep the per-block order exactly
            for (size_t i = 0; i < count; ++i) {
                static_vector<uint8_t> v(const_cast<uint8_t*>(payloads + i * _ds), _ds, _ds);
                auto r = writeBlock(v, DataLocation((int)(first + i), 0));
                if (!r && err)
                    err[i] = (uint8_t)r.error();
            }
            return {};
        }
        uint8_t* img = _disk.mapped(); // as readBlocks: a device without an engine takes the path it took
        if (img && ((size_t)first + count) * _raw > _disk.size())
            return unexpected(FsError::Disk_OutOfBounds);
        std::vector<uint8_t> raw(img ? 0 : count * _raw), status(count);
        if (!img) {
            auto rr = detail::disk_read(_disk, (size_t)first * _raw, count * _raw, raw.data());
            if (!rr)
                return unexpected(rr.error());
        }
        // the rows: in place on the disk image, or the copy just read
        if (!EccEngine::ok(
                ppfs_ecc_write_host(_eng.ctx(), payloads, img ? img + (size_t)first * _raw : raw.data(), status.data(), count),
                "write"))
            return unexpected(FsError::Disk_IOError);
        // a corrected old block's write-back is overwritten by the new block; blocks that failed their check
        // were left untouched by the engine
        report(status.data(), count, from(first), err);
        if (img)
            return {};
        auto w = detail::disk_write(_disk, (size_t)first * _raw, raw.data(), count * _raw);
        if (!w)
            return unexpected(w.error());
        return {};
    }

    // Lists.  With a mapped disk image (and no shortened RS code, whose write-back may run into
    // the next block): one ppfs_ecc_*_list_host call on the image, which gathers the listed rows,
    // cuts the list where an index repeats and copies the changed rows back.  Otherwise the rows are
    // read from the disk entry by entry, each stretch of the list without a repeated index goes
    // through one contiguous engine call, and the write-backs go to the disk in list order
    // (list_unmapped; a shortened RS code and a device without an engine take the per-block loop there).
    // The lists used to test for those two before they asked for the mapping and the other calls after;
    // mapped() only hands out an address, so the order cannot be told and engine_image() serves both.
    expected<void> readBlockList(const block_index_t* idx, size_t count, uint8_t* out, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        if (uint8_t* img = engine_image()) {
            std::vector<uint8_t> status(count);
            if (!EccEngine::ok(ppfs_ecc_decode_list_host(_eng.ctx(), img, _disk.size() / _raw, idx, count, out,
                                   status.data(), 1, nullptr),
                    "decode list"))
                return unexpected(FsError::Disk_IOError);
            report(status.data(), count, of(idx), err, out);
            return {};
        }
        std::vector<uint8_t> fixed, status, dec;
        return list_unmapped(
            idx, count,
            [&](size_t i, size_t n) { return IBlockDevice::readBlockList(idx + i, n, out + i * _ds, err ? err + i : nullptr); },
            [&](const std::vector<size_t>& pos, std::vector<uint8_t>& raw) {
                const size_t m = pos.size();
                fixed = raw;
                status.assign(m, 0);
                dec.assign(m * _ds, 0);
                if (!EccEngine::ok(ppfs_ecc_decode_host(_eng.ctx(), fixed.data(), dec.data(), status.data(), m, _wb, nullptr),
                        "decode"))
                    return false;
                for (size_t j = 0; j < m; ++j) {
                    const size_t i = pos[j];
                    if (const uint8_t e = status_error(status[j])) {
                        if (err)
                            err[i] = e;
                        std::memset(out + i * _ds, 0, _ds);
                        continue;
                    }
                    std::memcpy(out + i * _ds, dec.data() + j * _ds, _ds);
                    if (status[j] == PPFS_ECC_CORRECTED) {
                        auto wb = write_back(idx[i], raw.data() + j * _raw, fixed.data() + j * _raw, nullptr);
                        if (!wb && err)
                            err[i] = (uint8_t)wb.error();
                    }
                }
                return true;
            });
    }

    expected<void> writeBlockList(const block_index_t* idx, size_t count, const uint8_t* payloads, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        if (uint8_t* img = engine_image()) {
            std::vector<uint8_t> status(count);
            if (!EccEngine::ok(ppfs_ecc_write_list_host(_eng.ctx(), payloads, img, _disk.size() / _raw, idx,
                                   status.data(), count),
                    "write list"))
                return unexpected(FsError::Disk_IOError);
            report(status.data(), count, of(idx), err); // a corrected old block's write-back was overwritten by the new block
            return {};
        }
        std::vector<uint8_t> status, pay;
        return list_unmapped(
            idx, count,
            [&](size_t i, size_t n) { return IBlockDevice::writeBlockList(idx + i, n, payloads + i * _ds, err ? err + i : nullptr); },
            [&](const std::vector<size_t>& pos, std::vector<uint8_t>& raw) {
                const size_t m = pos.size();
                status.assign(m, 0);
                pay.resize(m * _ds);
                for (size_t j = 0; j < m; ++j)
                    std::memcpy(pay.data() + j * _ds, payloads + pos[j] * _ds, _ds);
                if (!EccEngine::ok(ppfs_ecc_write_host(_eng.ctx(), pay.data(), raw.data(), status.data(), m), "write"))
                    return false;
                for (size_t j = 0; j < m; ++j) {
                    const size_t i = pos[j];
                    if (const uint8_t e = status_error(status[j])) {
                        if (err)
                            err[i] = e; // block left untouched
                        continue;
                    }
                    if (status[j] == PPFS_ECC_CORRECTED)
                        log(idx[i]);
                    auto w = detail::disk_write(_disk, (size_t)idx[i] * _raw, raw.data() + j * _raw, _raw);
                    if (!w && err)
                        err[i] = (uint8_t)w.error();
                }
                return true;
            });
    }

    // Extents.  With a mapped disk image and no shortened RS code: one ppfs_ecc_*_extents_host call on
    // the image, which cuts the batch where a block repeats, so that two entries writing different
    // bytes of one block both land.  Otherwise the per-block loop.
    expected<void> readExtents(const ppfs_ecc_extent* ext, size_t n, uint8_t* out, size_t out_bytes, uint8_t* err) override
    {
        uint8_t* img = engine_image();
        if (!img || !n)
            return IBlockDevice::readExtents(ext, n, out, out_bytes, err);
        std::vector<uint8_t> status(n);
        if (!EccEngine::ok(ppfs_ecc_read_extents_host(_eng.ctx(), img, _disk.size() / _raw, ext, n, out, out_bytes,
                               status.data(), _wb),
                "read extents"))
            return unexpected(FsError::Disk_IOError);
        report(status.data(), n, of(ext), err);
        return {};
    }
    expected<void> writeExtents(const ppfs_ecc_extent* ext, size_t n, const uint8_t* in, size_t in_bytes, uint8_t* err) override
    {
        uint8_t* img = engine_image();
        if (!img || !n)
            return IBlockDevice::writeExtents(ext, n, in, in_bytes, err);
        std::vector<uint8_t> status(n);
        if (!EccEngine::ok(ppfs_ecc_write_extents_host(_eng.ctx(), in, in_bytes, img, _disk.size() / _raw, ext, n,
                               status.data()),
                "write extents"))
            return unexpected(FsError::Disk_IOError);
        report(status.data(), n, of(ext), err);
        return {};
    }

    // One engine call (ppfs_ecc_scrub_host) over the disk image from block `first` to the disk
    // end: the write-back of every corrected block is applied in index order, including RS
    // bytes a shortened code writes past a block end; corrected blocks are logged in order.
    expected<void> scrub(block_index_t first, size_t count, size_t* counts, uint8_t* err) override
    {
        if (err)
            std::memset(err, 0, count);
        const size_t base = (size_t)first * _raw;
        if (base + count * _raw > _disk.size())
            return unexpected(FsError::Disk_OutOfBounds);
        // in place on the disk image (the call handles a shortened code itself, so the mapping is all it asks
        // for); without one on a copy read from the disk, whose changed byte range goes back afterwards
        uint8_t* const img = _disk.mapped();
        const size_t bytes = _disk.size() - base;
        std::vector<uint8_t> copy(img ? 0 : bytes), before, status(count);
        if (!img) {
            auto rr = detail::disk_read(_disk, base, bytes, copy.data());
            if (!rr)
                return unexpected(rr.error());
            before = copy;
        }
        uint8_t* const image = img ? img + base : copy.data();
        size_t c3[3] = { 0, 0, 0 };
        if (!EccEngine::ok(ppfs_ecc_scrub_host(_eng.ctx(), image, bytes, count, status.data(), c3), "scrub"))
            return unexpected(FsError::Disk_IOError);
        report(status.data(), count, from(first), err);
        if (!img) {
            size_t lo = 0, hi = bytes;
            while (lo < hi && copy[lo] == before[lo])
                ++lo;
            while (hi > lo && copy[hi - 1] == before[hi - 1])
                --hi;
            if (hi > lo) {
                auto w = detail::disk_write(_disk, base + lo, copy.data() + lo, hi - lo);
                if (!w)
                    return unexpected(w.error());
            }
        }
        if (counts)
            std::memcpy(counts, c3, sizeof c3);
        return {};
    }

    // One engine call (ppfs_ecc_scrub_list_host) on a mapped disk image.  Elsewhere, and for a shortened RS
    // code, whose write-back may run into the next block, the per-block loop; its corrections are the
    // events the reads logged.
    expected<void> scrubList(const block_index_t* idx, size_t n, ppfs_ecc_scrub_counts* counts, uint8_t* err) override
    {
        uint8_t* img = engine_image();
        if (!img) {
            const size_t logged = _logged;
            ppfs_ecc_scrub_counts c {};
            auto r = IBlockDevice::scrubList(idx, n, &c, err);
            if (!r)
                return r;
            c.corrected = _logged - logged;
            c.ok -= std::min<uint64_t>(c.ok, c.corrected);
            if (counts)
                *counts = c;
            return {};
        }
        std::vector<uint8_t> status(n);
        ppfs_ecc_scrub_counts c {};
        if (!EccEngine::ok(ppfs_ecc_scrub_list_host(_eng.ctx(), img, _disk.size() / _raw, idx, n, status.data(), &c), "scrub list"))
            return unexpected(FsError::Disk_IOError);
        report(status.data(), n, of(idx), err);
        if (counts)
            *counts = c;
        return {};
    }

    // One engine call (ppfs_ecc_scrub_allocated_host) on a mapped disk image: the bitmap's blocks, then the
    // allocated blocks, each group's corrections logged in ascending block order as the reads would.
    expected<void> scrubAllocated(block_index_t bitmap_block, block_index_t first_data_block, size_t nbits,
        ppfs_ecc_scrub_counts* counts, uint8_t* err, uint8_t* bitmap_err) override
    {
        uint8_t* img = engine_image();
        if (!img || !_ds) {
            const size_t logged = _logged;
            ppfs_ecc_scrub_counts c {};
            auto r = IBlockDevice::scrubAllocated(bitmap_block, first_data_block, nbits, &c, err, bitmap_err);
            if (!r)
                return r;
            // scrubList above counted the data blocks' corrections; the rest were the bitmap's
            c.bitmap_corrected = _logged - logged - c.corrected;
            c.bitmap_ok -= std::min<uint64_t>(c.bitmap_ok, c.bitmap_corrected);
            if (counts)
                *counts = c;
            return {};
        }
        const size_t B = bitmapBlocks(nbits);
        std::vector<uint8_t> status(nbits), bst(B);
        ppfs_ecc_scrub_counts c {};
        if (!EccEngine::ok(ppfs_ecc_scrub_allocated_host(_eng.ctx(), img, _disk.size() / _raw, bitmap_block, first_data_block,
                               nbits, status.data(), bst.data(), &c),
                "scrub allocated"))
            return unexpected(FsError::Disk_OutOfBounds); // the only failures are the arguments': a range off the image
        report(bst.data(), B, from(bitmap_block), bitmap_err);
        report(status.data(), nbits, from(first_data_block), err); // a clear bit's 255 is no FsError and stays
        if (counts)
            *counts = c;
        return {};
    }

    // The file calls as engine calls on a mapped disk image: the whole tree in one ppfs_ecc_file_blocks_host (at
    // most three list decodes), for readFile followed by one ppfs_ecc_read_extents_host over the blocks whose
    // path held.  The result and the bytes equal the loop's; so does the log: each corrected index block's event
    // comes immediately before the event (if any) of the first requested file block under it, outer levels
    // first.  On a failing block the error and the byte count equal the loop's; blocks after the failing one may
    // additionally have been corrected and logged (the one deviation).  Elsewhere, for a shortened RS code and
    // for a range the loop refuses partway (past the file or the tree), the per-block loop.
    expected<void> fileBlocks(const ppfs_ecc_file& file, uint64_t first, size_t count, block_index_t* idx, uint8_t* err) override
    {
        FileBatch b(*this);
        b.add(0, file, first, count);
        if (!b.img)
            return IBlockDevice::fileBlocks(file, first, count, idx, err);
        if (!b.walk_one(idx))
            return unexpected(FsError::Disk_IOError);
        b.log(0);
        uint8_t e = 0;
        const size_t bad = b.first_failure(0, e);
        if (err) {
            std::memset(err, 0, bad);
            std::memset(err + bad, e, count - bad);
        }
        if (e)
            return unexpected((FsError)e);
        return {};
    }
    expected<size_t> readFile(const ppfs_ecc_file& file, size_t offset, size_t bytes_to_read, uint8_t* out,
        size_t* delivered = nullptr) override
    {
        if (bytes_to_read == 0 || _ds == 0 || offset >= file.file_size)
            return IBlockDevice::readFile(file, offset, bytes_to_read, out, delivered);
        const size_t n = std::min<size_t>(bytes_to_read, file.file_size - offset);
        FileBatch b(*this);
        b.add_range(0, file, offset, n);
        if (!b.img)
            return IBlockDevice::readFile(file, offset, bytes_to_read, out, delivered);
        if (!b.walk_one() || !b.read_extents(out, n, "read file extents")) // straight into the caller's buffer
            return unexpected(FsError::Disk_IOError);
        b.log(0);
        uint8_t e = 0;
        const size_t done = b.delivered(0, b.first_failure(0, e));
        if (delivered)
            *delivered = done;
        if (e)
            return unexpected((FsError)e);
        return n;
    }

    // readFiles as two engine calls on a mapped disk image: one ppfs_ecc_files_blocks_host over all the files'
    // trees (at most three list decodes whatever the number of files), one ppfs_ecc_read_extents_host over the
    // blocks whose path held.  Per file the result, the bytes and the log are readFile's, stop-at-first-failure
    // included; files are logged in batch order; blocks after a file's failing one may additionally have been
    // corrected and logged (readFile's one deviation).  Elsewhere, for a shortened RS code and when any range is
    // one the loop refuses partway, the loop over readFile.
    void readFiles(FileRead* reads, size_t n) override
    {
        auto by_range = [](const FileRead& r) { return r.bytes_to_read == 0 || r.offset >= r.file.file_size; };
        auto loop_one = [&](FileRead& r) { read_one(r, IBlockDevice::readFile(r.file, r.offset, r.bytes_to_read, r.out, &r.delivered)); };
        FileBatch b(*this);
        for (size_t i = 0; i < n; ++i)
            if (!by_range(reads[i])) // else answered from the range alone
                b.add_range(i, reads[i].file, reads[i].offset, std::min<size_t>(reads[i].bytes_to_read, reads[i].file.file_size - reads[i].offset));
        if (!b.img || b.sel.empty())
            return IBlockDevice::readFiles(reads, n);
        for (size_t i = 0; i < n; ++i)
            if (by_range(reads[i]))
                loop_one(reads[i]);
        auto fail_all = [&]() {
            for (const FileBatch::Span& s : b.sel) {
                reads[s.at].delivered = 0;
                read_one(reads[s.at], expected<size_t>(unexpected(FsError::Disk_IOError)));
            }
        };
        if (!b.walk(true))
            return fail_all();
        std::vector<uint8_t> buf(b.tot.bytes);
        for (size_t k = 0; k < b.sel.size(); ++k) // what no block writes stays the caller's
            std::memcpy(buf.data() + b.slots[k].out_pos, reads[b.sel[k].at].out, b.ranges[k].nbytes);
        if (!b.read_extents(buf.data(), buf.size(), "read files extents"))
            return fail_all();
        for (size_t k = 0; k < b.sel.size(); ++k) {
            FileRead& r = reads[b.sel[k].at];
            b.log(k);
            std::memcpy(r.out, buf.data() + b.slots[k].out_pos, b.ranges[k].nbytes);
            uint8_t e = 0;
            r.delivered = b.delivered(k, b.first_failure(k, e));
            read_one(r, e ? expected<size_t>(unexpected((FsError)e)) : expected<size_t>((size_t)b.ranges[k].nbytes));
        }
    }

    // readInodes as ONE ppfs_ecc_read_inodes_host on a mapped disk image.  Records and errors equal the loop's, and
    // so does the log, which piece_status makes possible: inodes in batch order, the bitmap block then the pieces up
    // to the first failing one, each block that some read of the call corrected logged where the loop first touches
    // it.  The pieces behind an inode's failing piece, which the loop does not read, have been read (and corrected)
    // as well: the one deviation.  Elsewhere, and for a shortened RS code, the per-inode loop.
    void readInodes(const InodeTable& table, const uint32_t* numbers, size_t n, InodeRead* out) override
    {
        uint8_t* img = engine_image();
        if (!img || !_ds || _ds > 0xFFFFu || !n)
            return IBlockDevice::readInodes(table, numbers, n, out);
        const size_t W = 1 + (2 + 79 / _ds);
        std::vector<ppfs_ecc_file> files(n);
        std::vector<ppfs_ecc_inode_meta> meta(n);
        std::vector<uint8_t> status(n), pieces(n * W);
        if (!EccEngine::ok(ppfs_ecc_read_inodes_host(_eng.ctx(), img, _disk.size() / _raw, &table, numbers, 4, n, files.data(),
                               meta.data(), status.data(), pieces.data(), nullptr, _wb),
                "read inodes")) {
            for (size_t j = 0; j < n; ++j) {
                out[j] = InodeRead {};
                out[j].error = FsError::Disk_IOError;
            }
            return;
        }
        inode_log(table, numbers, n, pieces.data());
        for (size_t j = 0; j < n; ++j) {
            InodeRead& r = out[j];
            r = InodeRead {};
            if (!(r.ok = inode_ok(table, numbers[j], status[j], r.error)))
                continue;
            r.inode.time_creation = meta[j].time_creation;
            r.inode.time_modified = meta[j].time_modified;
            r.inode.file = files[j];
            r.inode.type = meta[j].type;
        }
    }

    // lookupNames / lookupInodes as ONE ppfs_ecc_lookup_host on a mapped disk image, behind the FileBatch walk of the
    // directories' trees that the log needs (which image block each file block and index block is).  Results equal
    // the loop's for every query.  The log holds the loop's events first and in the loop's order: queries in order,
    // each block at its first read, an index block in front of the first file block under it.  The engine reads every
    // directory whole, so directory blocks that no query's loop reached -- behind last(B), or behind a failing block
    // -- may additionally have been corrected; they are logged after the loop's events in (directory, block) order,
    // and the disk is the loop's with exactly those blocks corrected as well: readFile's deviation.  Elsewhere, for a
    // shortened RS code and for a directory past its tree's capacity, the loop.
    void lookupNames(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq) override { lookup_engine(dirs, ndirs, queries, nq, true); }
    void lookupInodes(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq) override { lookup_engine(dirs, ndirs, queries, nq, false); }
    void lookup_engine(const ppfs_ecc_file* dirs, size_t ndirs, Lookup* queries, size_t nq, bool by_name)
    {
        auto loop = [&]() { IBlockDevice::lookup_loop(dirs, ndirs, queries, nq, by_name); };
        if (!nq || _ds > 0xFFFFu)
            return loop();
        // the directories that have entries, as a batch of ranges (0, 128 n); slot[d]: directory d's number in it
        FileBatch b(*this);
        std::vector<uint32_t> slot(ndirs, 0xFFFFFFFFu);
        for (size_t d = 0; d < ndirs; ++d) {
            const size_t n = dirs[d].file_size / kDirEntryBytes;
            if (n) {
                slot[d] = (uint32_t)b.sel.size();
                b.add_range(d, dirs[d], 0, n * kDirEntryBytes);
            }
        }
        for (size_t q = 0; q < nq; ++q)
            if (queries[q].dir >= ndirs)
                return loop();
        if (!b.img)
            return loop();
        if (b.sel.empty()) // nothing to read: the loop answers from the sizes alone
            return loop();
        auto fail_all = [&]() {
            for (size_t q = 0; q < nq; ++q) {
                queries[q].ok = false;
                queries[q].error = FsError::Disk_IOError;
                queries[q].inode = queries[q].entry = 0xFFFFFFFFu;
            }
        };
        if (!b.walk(true))
            return fail_all();
        // the engine gets the queries on directories that have entries; at[q]: query q's number among them
        std::vector<size_t> at(nq, (size_t)-1);
        std::vector<ppfs_ecc_lookup_query> qs;
        std::vector<uint8_t> names;
        for (size_t q = 0; q < nq; ++q) {
            if (slot[queries[q].dir] == 0xFFFFFFFFu)
                continue; // an empty directory: not found, nothing read
            at[q] = qs.size();
            qs.push_back(ppfs_ecc_lookup_query { slot[queries[q].dir], queries[q].key });
            if (by_name)
                names.insert(names.end(), queries[q].name, queries[q].name + 128);
        }
        std::vector<ppfs_ecc_lookup_hit> hits(qs.size());
        std::vector<uint8_t> entries(b.tot.bytes + 1);
        if (!EccEngine::ok(ppfs_ecc_lookup_host(_eng.ctx(), b.img, _disk.size() / _raw, b.files.data(), b.files.size(), qs.data(),
                               by_name ? names.data() : nullptr, qs.size(), by_name ? 0 : 1, entries.data(), b.tot.bytes, b.status.data(),
                               nullptr, hits.data(), nullptr, nullptr, _wb),
                "lookup"))
            return fail_all();
        // per directory its corrected blocks in the loop's order, and its first failing file block
        std::vector<std::vector<FileEvent>> events(b.sel.size());
        std::vector<size_t> cursor(b.sel.size(), 0), failing(b.sel.size());
        for (size_t k = 0; k < b.sel.size(); ++k) {
            const ppfs_ecc_files_slot& t = b.slots[k];
            std::vector<uint64_t> under[3];
            file_tree_under(0, b.sel[k].count, under);
            for (int d = 0; d < 3; ++d)
                for (size_t i = 0; i < under[d].size() && i < t.tree_n[d]; ++i)
                    if (b.tst[t.tree_pos[d] + i] == PPFS_ECC_CORRECTED)
                        events[k].push_back(FileEvent { under[d][i], d, b.tidx[t.tree_pos[d] + i] });
            for (size_t i = 0; i < b.sel[k].count; ++i)
                if (b.status[t.block_pos + i] == PPFS_ECC_CORRECTED)
                    events[k].push_back(FileEvent { i, 3, b.idx[t.block_pos + i] });
            std::stable_sort(events[k].begin(), events[k].end(),
                [](const FileEvent& x, const FileEvent& y) { return x.at != y.at ? x.at < y.at : x.level < y.level; });
            uint8_t e = 0;
            failing[k] = b.first_failure(k, e);
        }
        auto log_upto = [&](size_t k, uint64_t last) { // the loop's reads of file blocks [0, last] of directory k
            for (; cursor[k] < events[k].size() && events[k][cursor[k]].at <= last; ++cursor[k])
                log(events[k][cursor[k]].block);
        };
        for (size_t q = 0; q < nq; ++q) {
            Lookup& r = queries[q];
            const ppfs_ecc_lookup_hit h = at[q] != (size_t)-1 ? hits[at[q]] : ppfs_ecc_lookup_hit { 0xFFFFFFFFu, 0xFFFFFFFFu, PPFS_ECC_NOT_FOUND, 0 };
            const size_t n = dirs[r.dir].file_size / kDirEntryBytes;
            if (n) {
                const size_t k = slot[r.dir], B = h.status == PPFS_ECC_OK ? h.entry / kDirEntryBatch : (n - 1) / kDirEntryBatch;
                const uint64_t last = (std::min((B + 1) * kDirEntryBatch, n) * kDirEntryBytes - 1) / _ds;
                log_upto(k, std::min<uint64_t>(last, failing[k]));
            }
            r.ok = n && h.status == PPFS_ECC_OK;
            r.inode = r.ok ? h.inode : 0xFFFFFFFFu;
            r.entry = r.ok ? h.entry : 0xFFFFFFFFu;
            r.error = r.ok                                     ? FsError {}
                : !n || h.status == PPFS_ECC_NOT_FOUND ? (by_name ? FsError::PpFS_NotFound : FsError::DirectoryManager_NotFound)
                                                       : (FsError)status_error((uint8_t)h.status);
        }
        for (size_t k = 0; k < b.sel.size(); ++k) // what the engine corrected beyond the loop's reach
            log_upto(k, ~0ull);
    }

    // writeInodes as ONE ppfs_ecc_write_inodes_host on a mapped disk image, from the steps readInodes is made of.
    // Errors equal the loop's, and so does the log: the first toucher of a corrected block reports it, and the log
    // replays the loop's order up to each inode's first failing piece.  The pieces behind an inode's failing piece,
    // which the loop does not write, have been written as well: the one deviation.  Elsewhere, and for a shortened
    // RS code, the per-inode loop.
    void writeInodes(const InodeTable& table, const uint32_t* numbers, size_t n, const PackedInode* inodes, InodeWrite* out) override
    {
        uint8_t* img = engine_image();
        if (!img || !_ds || _ds > 0xFFFFu || !n)
            return IBlockDevice::writeInodes(table, numbers, n, inodes, out);
        const size_t W = 1 + (2 + 79 / _ds);
        std::vector<ppfs_ecc_file> files(n);
        std::vector<ppfs_ecc_inode_meta> meta(n);
        for (size_t j = 0; j < n; ++j) {
            files[j] = inodes[j].file;
            meta[j] = ppfs_ecc_inode_meta { inodes[j].time_creation, inodes[j].time_modified, inodes[j].type, {} };
        }
        std::vector<uint8_t> status(n), pieces(n * W);
        if (!EccEngine::ok(ppfs_ecc_write_inodes_host(_eng.ctx(), img, _disk.size() / _raw, &table, numbers, 4, n, files.data(),
                               meta.data(), status.data(), pieces.data(), nullptr, _wb),
                "write inodes")) {
            std::fill(out, out + n, InodeWrite { false, FsError::Disk_IOError });
            return;
        }
        inode_log(table, numbers, n, pieces.data());
        for (size_t j = 0; j < n; ++j) {
            out[j] = InodeWrite {};
            out[j].ok = inode_ok(table, numbers[j], status[j], out[j].error);
        }
    }

    // writeFile / writeFiles as engine calls on a mapped disk image: one ppfs_ecc_files_blocks_host over all the
    // files' trees -- the write call reports the tree only as counts, and the log needs to know WHICH index blocks
    // were corrected -- then ONE ppfs_ecc_write_files_host.  Per file the result, `written` and the log up to the
    // first failing block are the loop's; files are logged in batch order, index blocks in readFile's order.
    // Every block of every range is attempted, so blocks after a file's failing one have been written (and
    // logged) as well: the one deviation.  Elsewhere, for a shortened RS code and when any range is one the loop
    // refuses partway, the per-block loop.
    expected<size_t> writeFile(const ppfs_ecc_file& file, size_t offset, const uint8_t* in, size_t n, size_t* written = nullptr) override
    {
        FileWrite w { file, offset, in, n, false, FsError {}, 0, 0 };
        writeFiles(&w, 1);
        if (written)
            *written = w.written;
        if (!w.ok)
            return unexpected(w.error);
        return w.bytes;
    }
    void writeFiles(FileWrite* writes, size_t n) override
    {
        auto by_range = [](const FileWrite& w) { return w.n == 0 || w.offset + w.n < w.offset || w.offset + w.n > w.file.file_size; };
        auto loop_one = [&](FileWrite& w) { write_one(w, IBlockDevice::writeFile(w.file, w.offset, w.in, w.n, &w.written)); };
        FileBatch b(*this);
        for (size_t i = 0; i < n; ++i)
            if (!by_range(writes[i])) // else answered from the range alone
                b.add_range(i, writes[i].file, writes[i].offset, writes[i].n);
        if (!b.img || b.sel.empty()) {
            for (size_t i = 0; i < n; ++i)
                loop_one(writes[i]);
            return;
        }
        for (size_t i = 0; i < n; ++i)
            if (by_range(writes[i]))
                loop_one(writes[i]);
        auto fail_all = [&]() {
            for (const FileBatch::Span& s : b.sel) {
                writes[s.at].written = 0;
                write_one(writes[s.at], expected<size_t>(unexpected(FsError::Disk_IOError)));
            }
        };
        if (!b.walk(false)) // no path statuses: the write's own status holds the path's where that is non-zero
            return fail_all();
        const size_t m = b.sel.size();
        std::vector<uint8_t> buf(b.tot.bytes);
        std::vector<uint64_t> done(m, 0);
        for (size_t k = 0; k < m; ++k)
            std::memcpy(buf.data() + b.slots[k].out_pos, writes[b.sel[k].at].in, writes[b.sel[k].at].n);
        if (!EccEngine::ok(ppfs_ecc_write_files_host(_eng.ctx(), buf.data(), buf.size(), b.img, _disk.size() / _raw, b.files.data(),
                               b.ranges.data(), m, b.status.data(), nullptr, done.data(), nullptr, _wb),
                "write files"))
            return fail_all();
        for (size_t k = 0; k < m; ++k) {
            FileWrite& w = writes[b.sel[k].at];
            b.log(k);
            w.written = (size_t)done[k];
            uint8_t e = 0;
            b.first_failure(k, e);
            write_one(w, e ? expected<size_t>(unexpected((FsError)e)) : expected<size_t>(w.n));
        }
    }

protected:
    // a corrected block of a file call: the file block it is read before (itself, for a data block), its level
    // (0-2: the tree's, 3: data) and its image block
    struct FileEvent {
        uint64_t at;
        int level;
        block_index_t block;
    };
    // the tree's entries of a walk over [first, first + count), per level in level order (ppfs_ecc.h), as the first
    // requested file block under each: a new index block at depth d starts where the slots above the block's own change
    void file_tree_under(uint64_t first, size_t count, std::vector<uint64_t> (&under)[3]) const
    {
        const uint64_t ipb = _ds / 4;
        FilePath prev { 4, { 0, 0, 0 } };
        for (uint64_t j = first; j < first + count; ++j) {
            const FilePath p = file_path(j, ipb);
            bool fresh = p.segment != prev.segment;
            for (unsigned d = 0; d < p.segment; ++d) {
                if (d > 0)
                    fresh = fresh || p.slot[d - 1] != prev.slot[d - 1];
                if (fresh)
                    under[d].push_back(j);
            }
            prev = p;
        }
    }

    // A batch of file ranges for the engine on the mapped image -- one range for fileBlocks and readFile.  Its
    // three parts: which of a call's entries the engine takes (add: all of them or none); the files / ranges /
    // slots arrays with the plan and the walk of all the trees, whose results lie in the per-block and per-tree-
    // block arrays as ppfs_ecc_files_plan says (walk; walk_one is the single-file calls, its one slot filled in
    // here); and per file its correction events, its first failing block and the bytes before that one.
    struct FileBatch {
        struct Span { // an entry the engine takes: its number in the call and its file blocks
            size_t at;
            uint64_t first;
            size_t count;
        };
        EngineBlockDevice& dev;
        uint8_t* img; // null: the call takes the per-block loop
        std::vector<Span> sel;
        std::vector<ppfs_ecc_file> files;
        std::vector<ppfs_ecc_file_range> ranges;
        std::vector<ppfs_ecc_files_slot> slots;
        ppfs_ecc_files_totals tot {};
        block_index_t* idx = nullptr; // own_idx, or the caller's array
        std::vector<block_index_t> own_idx, tidx;
        std::vector<uint8_t> path, tst, status; // path: empty unless the walk was asked for it; status: the data blocks'
        std::vector<ppfs_ecc_extent> all;       // read_extents: every file block's extent, pos in the packed buffer

        explicit FileBatch(EngineBlockDevice& d)
            : dev(d)
            , img(d._ds ? d.engine_image() : nullptr)
        {
        }
        // Entry `at` of the call is the file blocks [first, first + count), the bytes `range`.  The engine takes
        // it unless the loop refuses the range partway (past the file or the tree); then img becomes null.
        void add(size_t at, const ppfs_ecc_file& file, uint64_t first, size_t count, ppfs_ecc_file_range range = { 0, 0 })
        {
            if (!img)
                return;
            if (!count || first + count > file_occupied(file, dev._ds) || file_path(first + count - 1, dev._ds / 4).segment > 3)
                img = nullptr;
            sel.push_back(Span { at, first, count });
            files.push_back(file);
            ranges.push_back(range);
        }
        void add_range(size_t at, const ppfs_ecc_file& file, size_t offset, size_t nbytes)
        {
            if (img)
                add(at, file, offset / dev._ds, (offset % dev._ds + nbytes + dev._ds - 1) / dev._ds, ppfs_ecc_file_range { offset, nbytes });
        }
        // the plan, then all the trees in one engine call; false when the engine refuses
        bool walk(bool want_path)
        {
            const size_t m = sel.size();
            slots.resize(m);
            if (!EccEngine::ok(ppfs_ecc_files_plan(dev._eng.ctx(), files.data(), ranges.data(), m, slots.data(), &tot), "files plan"))
                return false;
            own_idx.resize(tot.blocks);
            idx = own_idx.data();
            tidx.resize(tot.tree_blocks);
            tst.resize(tot.tree_blocks);
            status.assign(tot.blocks, 0);
            if (want_path)
                path.resize(tot.blocks);
            return EccEngine::ok(ppfs_ecc_files_blocks_host(dev._eng.ctx(), img, dev._disk.size() / dev._raw, files.data(),
                                     ranges.data(), m, idx, want_path ? path.data() : nullptr, tidx.data(), tst.data(), nullptr,
                                     nullptr, dev._wb),
                "files blocks");
        }
        // the one file through the single-file calls, its blocks into `into` if given
        bool walk_one(block_index_t* into = nullptr)
        {
            const Span& s = sel[0];
            const long long T = ppfs_ecc_file_tree_blocks(dev._eng.ctx(), &files[0], s.first, s.count);
            if (T < 0)
                return false;
            own_idx.resize(into ? 0 : s.count);
            idx = into ? into : own_idx.data();
            tidx.resize((size_t)T);
            tst.resize((size_t)T);
            path.resize(s.count);
            status.assign(s.count, 0);
            if (!EccEngine::ok(ppfs_ecc_file_blocks_host(dev._eng.ctx(), img, dev._disk.size() / dev._raw, &files[0], s.first, s.count,
                                   idx, path.data(), tidx.data(), tst.data(), nullptr, dev._wb),
                    "file blocks"))
                return false;
            // its tree entries lie level after level, as many per level as the walk below expects
            std::vector<uint64_t> under[3];
            dev.file_tree_under(s.first, s.count, under);
            slots.assign(1, ppfs_ecc_files_slot {});
            size_t k = 0;
            for (int d = 0; d < 3; ++d) {
                slots[0].tree_pos[d] = k;
                slots[0].tree_n[d] = under[d].size();
                k += under[d].size();
            }
            return k == (size_t)T;
        }
        // One ppfs_ecc_read_extents_host over the blocks whose path held, file k's bytes at out + its out_pos;
        // their statuses go to `status`.  false when the engine refuses.
        bool read_extents(uint8_t* out, size_t out_bytes, const char* what)
        {
            for (size_t k = 0; k < sel.size(); ++k)
                for (ppfs_ecc_extent e : file_extents(idx + slots[k].block_pos, sel[k].count, ranges[k].offset % dev._ds, ranges[k].nbytes, dev._ds)) {
                    e.pos += slots[k].out_pos;
                    all.push_back(e);
                }
            if (all.size() != status.size()) // one extent per block of the walk
                return false;
            std::vector<ppfs_ecc_extent> live;
            std::vector<size_t> live_at;
            for (size_t i = 0; i < all.size(); ++i)
                if (!path[i]) {
                    live.push_back(all[i]);
                    live_at.push_back(i);
                }
            if (live.empty())
                return true;
            std::vector<uint8_t> st(live.size());
            if (!EccEngine::ok(ppfs_ecc_read_extents_host(dev._eng.ctx(), img, dev._disk.size() / dev._raw, live.data(), live.size(), out,
                                   out_bytes, st.data(), dev._wb),
                    what))
                return false;
            for (size_t k = 0; k < live.size(); ++k)
                status[live_at[k]] = st[k];
            return true;
        }
        // File k's corrected blocks, logged in the loop's order: an index block immediately before the first
        // requested file block under it, outer levels first, then that block itself.
        void log(size_t k)
        {
            const Span& s = sel[k];
            const ppfs_ecc_files_slot& t = slots[k];
            std::vector<FileEvent> events;
            std::vector<uint64_t> under[3];
            dev.file_tree_under(s.first, s.count, under);
            for (int d = 0; d < 3; ++d)
                for (size_t i = 0; i < under[d].size() && i < t.tree_n[d]; ++i)
                    if (tst[t.tree_pos[d] + i] == PPFS_ECC_CORRECTED)
                        events.push_back(FileEvent { under[d][i], d, tidx[t.tree_pos[d] + i] });
            for (size_t i = 0; i < s.count; ++i)
                if (status[t.block_pos + i] == PPFS_ECC_CORRECTED)
                    events.push_back(FileEvent { s.first + i, 3, idx[t.block_pos + i] });
            std::stable_sort(events.begin(), events.end(),
                [](const FileEvent& a, const FileEvent& b) { return a.at != b.at ? a.at < b.at : a.level < b.level; });
            for (const FileEvent& e : events)
                dev.log(e.block);
        }
        // File k's first failing block, counted from its first, and that block's error (its path's, else its own)
        // in e; its count and 0 when none fails.
        size_t first_failure(size_t k, uint8_t& e) const
        {
            for (size_t i = 0; i < sel[k].count; ++i) {
                const size_t at = slots[k].block_pos + i;
                e = !path.empty() && path[at] ? path[at] : status_error(status[at]);
                if (e)
                    return i;
            }
            e = 0;
            return sel[k].count;
        }
        // the bytes of file k that lie before its block i (after read_extents)
        size_t delivered(size_t k, size_t i) const
        {
            return i < sel[k].count ? (size_t)(all[slots[k].block_pos + i].pos - slots[k].out_pos) : (size_t)ranges[k].nbytes;
        }
    };

    EngineBlockDevice(IDisk& disk, std::shared_ptr<Logger> logger, uint32_t type, uint32_t bs, uint32_t t,
        uint64_t poly, int device, const char* log_name)
        : _disk(disk)
        , _logger(std::move(logger))
        , _type(type)
        , _wb(type == PPFS_ECC_REED_SOLOMON || type == PPFS_ECC_HAMMING ? 1 : 0)
        , _eng(type, bs, t, poly, device)
        , _raw(_eng.raw())
        , _ds(_eng.data())
        , _log_name(log_name)
    {
    }

    bool has_spill() const { return _type == PPFS_ECC_REED_SOLOMON && _raw > 0 && _raw < 255; }
    size_t spill_stride() const { return 256 - std::min<size_t>(_raw, 255); }

    // the end of the stretch of a list from `start` in which no index repeats
    static size_t list_run_end(const block_index_t* idx, size_t count, size_t start)
    {
        std::unordered_set<block_index_t> seen;
        size_t e = start;
        while (e < count && seen.insert(idx[e]).second)
            ++e;
        return e;
    }
    // The rows of the entries [s, e) that lie on the disk, packed in list order, and their list
    // positions; false when a row on the disk could not be read.
    bool list_rows(const block_index_t* idx, size_t s, size_t e, std::vector<size_t>& pos, std::vector<uint8_t>& rows)
    {
        pos.clear();
        for (size_t i = s; i < e; ++i)
            if (((size_t)idx[i] + 1) * _raw <= _disk.size())
                pos.push_back(i);
        rows.assign(pos.size() * _raw, 0);
        for (size_t j = 0; j < pos.size(); ++j)
            if (!detail::disk_read(_disk, (size_t)idx[pos[j]] * _raw, _raw, rows.data() + j * _raw))
                return false;
        return true;
    }
    // A list on a disk without a mapping, for readBlockList and writeBlockList.  Each stretch without a repeated
    // index: its rows read from the disk; per_block(i, n), the per-block loop over the entries [i, i + n), for
    // the whole stretch when a row could not be read and else for its entries off the disk; then packed(pos,
    // rows), the call's one contiguous engine call on the packed rows and its epilogue per row in list order,
    // false when the engine refuses.  A shortened RS code and a device without an engine take the per-block loop.
    template <class PerBlock, class Packed>
    expected<void> list_unmapped(const block_index_t* idx, size_t count, PerBlock per_block, Packed packed)
    {
        if (has_spill() || !_raw)
            return per_block(0, count);
        std::vector<uint8_t> raw;
        std::vector<size_t> pos;
        for (size_t s = 0; s < count;) {
            const size_t e = list_run_end(idx, count, s);
            if (!list_rows(idx, s, e, pos, raw)) { // a row could not be read: block by block
                auto r = per_block(s, e - s);
                if (!r)
                    return r;
                s = e;
                continue;
            }
            for (size_t i = s, j = 0; i < e; ++i) { // off the disk: the per-block call's error
                if (j < pos.size() && pos[j] == i) {
                    ++j;
                    continue;
                }
                auto r = per_block(i, 1);
                if (!r)
                    return r;
            }
            if (!pos.empty() && !packed(pos, raw))
                return unexpected(FsError::Disk_IOError);
            s = e;
        }
        return {};
    }

    void log(block_index_t b)
    {
        ++_logged;
        if (_logger && _log_name)
            _logger->logEvent(ErrorCorrectionEvent(_log_name, b));
    }

    // The reference's write-back of a corrected block (old = raw as read, fixed = corrected).
    expected<void> write_back(block_index_t b, const uint8_t* old, const uint8_t* fixed, const uint8_t* spill)
    {
        if (_type == PPFS_ECC_REED_SOLOMON) {
            // rs_block_device.cpp:171-180: log, then write the whole corrected codeword (and,
            // for shortened codes, what its polynomial holds past n); the result is ignored
            log(b);
            std::vector<uint8_t> wbuf(fixed, fixed + _raw);
            if (spill && spill[0])
                wbuf.insert(wbuf.end(), spill + 1, spill + 1 + spill[0]);
            (void)detail::disk_write(_disk, (size_t)b * _raw, wbuf.data(), wbuf.size());
            return {};
        }
        // hamming_block_device.cpp:41-57: write back only the flipped byte, then log
        size_t byte = 0;
        while (byte < _raw && old[byte] == fixed[byte])
            ++byte;
        if (byte == _raw)
            byte = 0;
        auto w = detail::disk_write(_disk, (size_t)b * _raw + byte, fixed + byte, 1);
        if (!w)
            return unexpected(w.error());
        log(b);
        return {};
    }

    // _fixBlockAndExtract / _readAndCheckRaw / _readAndFixBlock for one block; raw is replaced
    // by the (fixed) old block, dec receives the payload.
    expected<void> check_fix(block_index_t b, uint8_t* raw, uint8_t* dec)
    {
        std::vector<uint8_t> fixed(raw, raw + _raw), spill;
        uint8_t status = 0;
        if (has_spill())
            spill.assign(spill_stride(), 0);
        if (!EccEngine::ok(ppfs_ecc_decode_host(_eng.ctx(), fixed.data(), dec, &status, 1, _wb,
                               spill.empty() ? nullptr : spill.data()),
                "decode"))
            return unexpected(FsError::Disk_IOError);
        if (status == PPFS_ECC_CORRECTION_ERROR)
            return unexpected(FsError::BlockDevice_CorrectionError);
        if (status == PPFS_ECC_CORRECTED && _wb) {
            auto w = write_back(b, raw, fixed.data(), spill.empty() ? nullptr : spill.data());
            if (!w)
                return w;
        }
        std::memcpy(raw, fixed.data(), _raw);
        return {};
    }

    IDisk& _disk;
    std::shared_ptr<Logger> _logger;
    uint32_t _type;
    const int _wb; // the engine calls' write_back: RS and Hamming write a corrected block back, CRC and parity only detect
    EccEngine _eng;
    size_t _raw, _ds;
    const char* _log_name;
    size_t _logged = 0; // correction events so far (log()): what a per-block scrub loop corrected
};

class ReedSolomonBlockDevice : public EngineBlockDevice {
public:
    // raw_block_size is clamped to 255 and correctable_bytes to raw/2 (rs_block_device.cpp:52-60)
    ReedSolomonBlockDevice(IDisk& disk, size_t raw_block_size, size_t correctable_bytes,
        std::shared_ptr<Logger> logger = nullptr, int device = 0)
        : EngineBlockDevice(disk, std::move(logger), PPFS_ECC_REED_SOLOMON, (uint32_t)raw_block_size,
            (uint32_t)correctable_bytes, 0, device, "ReedSolomon")
    {
    }
};

class CrcBlockDevice : public EngineBlockDevice {
public:
    CrcBlockDevice(CrcPolynomial polynomial, IDisk& disk, size_t block_size, std::shared_ptr<Logger> logger = nullptr,
        int device = 0)
        : EngineBlockDevice(disk, std::move(logger), PPFS_ECC_CRC, (uint32_t)block_size, 0,
            polynomial.getExplicitPolynomial(), device, nullptr)
    {
    }
};

class HammingBlockDevice : public EngineBlockDevice {
public:
    HammingBlockDevice(int block_size_power, IDisk& disk, std::shared_ptr<Logger> logger = nullptr, int device = 0)
        : EngineBlockDevice(disk, std::move(logger), PPFS_ECC_HAMMING, 1u << block_size_power, 0, 0, device,
            "Hamming")
    {
    }
};

class ParityBlockDevice : public EngineBlockDevice {
public:
    ParityBlockDevice(int block_size, IDisk& disk, std::shared_ptr<Logger> logger = nullptr, int device = 0)
        : EngineBlockDevice(disk, std::move(logger), PPFS_ECC_PARITY, (uint32_t)block_size, 0, 0, device, nullptr)
    {
    }
};

} // namespace ppfs_gpu
